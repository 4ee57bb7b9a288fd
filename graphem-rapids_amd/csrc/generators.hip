// Graph generators on the GPU and on the host (include/graphem_hip.h "graph generators"; graphem-rapids_amd/generators.py).
//
// The three random rules of the header are written once as __host__ __device__ functions over integers; a device handle
// runs them in kernels, a host handle (device_id < 0) in plain loops, and both end in the same sorted key list.
//
//   block model   one work item per segment of a block pair's pair space: gen_sbm_kernel<false> counts the segment's
//                 edges, hipCUB scans the counts, gen_sbm_kernel<true> walks the segment again and writes its keys.
//   geometric     gen_geo_points_kernel (coordinates, cell of the first min(dim, 3) of them), radix sort by cell,
//                 gen_geo_gather_kernel (coordinates in cell order), gen_geo_cells_kernel (first point of every cell),
//                 gen_geo_pairs_kernel<false / true>: one lane per point over the 3^(g-1) runs of three neighbour cells
//                 (cells that differ in the last grid axis are adjacent in memory), integer distance over all dim.
//   attachment    gen_ba_round_kernel once per round over the list of unfinished vertices; a vertex reads the targets of
//                 another only when that one finished in an earlier launch, else it stops at that draw and is listed for
//                 the next round.  The host reads the length of that list after every launch.
// All three finish with a 64-bit radix sort of u << 32 | v and gen_unpack_kernel (keys -> int32 pairs).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_util.h"

#define GEN_GOLDEN 0x9E3779B97F4A7C15ull
#define GEN_BLOCK 256
#define GEN_MAX_BLOCKS 65536
#define GEN_DEFAULT_BUDGET (4ll << 30)
#define GEN_SEG GH_GEN_SBM_SEGMENT
#define GEN_TAB GH_GEN_SBM_TABLE
#define GEN_MAX_DIM 8
#define GEN_COORD_ONE (1u << 24)

namespace {

__host__ __device__ __forceinline__ uint64_t gen_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t gen_stream(uint64_t seed, uint64_t i) { return gen_mix(seed + (i + 1) * GEN_GOLDEN); }
__host__ __device__ __forceinline__ uint64_t gen_word(uint64_t stream, uint64_t j) { return gen_mix(stream ^ j); }

__host__ __device__ __forceinline__ uint64_t gen_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

__host__ __device__ __forceinline__ uint64_t gen_key(int64_t u, int64_t v) {
    return u < v ? ((uint64_t)u << 32) | (uint64_t)v : ((uint64_t)v << 32) | (uint64_t)u;
}

// ---- block model ------------------------------------------------------------------------------------------------
struct SbmPair {          // one block pair (a <= b)
    int64_t seg0;         // its first segment
    int64_t N;            // size of its pair space
    int64_t off_a, off_b, s_a, s_b;
    int32_t table;        // row of the gap tables, -1: p == 0
    int32_t diag;         // a == b
};

__host__ __device__ __forceinline__ uint64_t sbm_pair_key(const SbmPair &bp, int64_t i) {
    if (!bp.diag) return gen_key(bp.off_a + i / bp.s_b, bp.off_b + i % bp.s_b);
    const int64_t s = bp.s_a, h = (s - 1) / 2;
    if (i < s * h) {
        const int64_t r = i / h, c = i % h;
        return gen_key(bp.off_a + r, bp.off_a + (r + 1 + c) % s);
    }
    const int64_t r = i - s * h;
    return gen_key(bp.off_a + r, bp.off_a + r + s / 2);
}

// Walks segment g; emit(key) per edge.  Returns the number of edges.
template <class Emit>
__host__ __device__ __forceinline__ int64_t sbm_walk(int64_t g, uint64_t seed, const SbmPair *pairs, int64_t n_pairs,
                                                      const uint64_t *tables, Emit emit) {
    // the last block pair with seg0 <= g: a block pair without segments shares seg0 with its successor, so this is the owner
    int64_t lo = 0, hi = n_pairs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (pairs[mid].seg0 <= g) lo = mid; else hi = mid - 1;
    }
    const SbmPair bp = pairs[lo];
    if (bp.table < 0) return 0;
    const uint64_t *cdf = tables + (int64_t)bp.table * GEN_TAB;
    int64_t pos = (g - bp.seg0) * GEN_SEG;
    const int64_t end = bp.N - pos < GEN_SEG ? bp.N : pos + GEN_SEG;
    const uint64_t stream = gen_stream(seed, (uint64_t)g);
    int64_t count = 0;
    for (uint64_t j = 0; pos < end; ++j) {
        const uint64_t r = gen_word(stream, j) >> 12;
        int a = 0, b = GEN_TAB;               // the number of entries <= r
        while (a < b) {
            const int mid = (a + b) / 2;
            if (cdf[mid] <= r) a = mid + 1; else b = mid;
        }
        if (a == GEN_TAB) { pos += GEN_TAB; continue; }
        pos += a;
        if (pos < end) { emit(sbm_pair_key(bp, pos), count); ++count; }
        pos += 1;
    }
    return count;
}

struct EmitNone { __host__ __device__ void operator()(uint64_t, int64_t) const {} };
struct EmitAt {
    uint64_t *out;
    __host__ __device__ void operator()(uint64_t key, int64_t i) const { out[i] = key; }
};

template <bool WRITE>
__global__ __launch_bounds__(GEN_BLOCK) void gen_sbm_kernel(int64_t n_segments, uint64_t seed, const SbmPair *__restrict__ pairs,
                                                           int64_t n_pairs, const uint64_t *__restrict__ tables,
                                                           int64_t *counts, const int64_t *__restrict__ offsets, uint64_t *keys) {
    for (int64_t g = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x; g < n_segments; g += (int64_t)gridDim.x * GEN_BLOCK) {
        if (WRITE) sbm_walk(g, seed, pairs, n_pairs, tables, EmitAt{keys + offsets[g]});
        else counts[g] = sbm_walk(g, seed, pairs, n_pairs, tables, EmitNone{});
    }
}

// ---- geometric ----------------------------------------------------------------------------------------------------
struct GeoGrid {
    int32_t dim, gdim;      // coordinates; grid axes = min(dim, 3)
    uint32_t side, ncell;   // cell side in coordinate units (>= the integer radius), cells per axis
    uint64_t R2;
};

__host__ __device__ __forceinline__ uint32_t geo_coord(uint64_t stream, int d) { return (uint32_t)(gen_word(stream, (uint64_t)d) >> 40); }

__host__ __device__ __forceinline__ uint32_t geo_cell(const GeoGrid &g, const uint32_t *k) {
    uint32_t c = 0;
    for (int d = 0; d < g.gdim; ++d) c = c * g.ncell + k[d] / g.side;
    return c;
}

__global__ __launch_bounds__(GEN_BLOCK) void gen_geo_points_kernel(int64_t n, uint64_t seed, GeoGrid g, uint32_t *coords, float *pos,
                                                                  uint32_t *cell, uint32_t *ids) {
    const int64_t i = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t stream = gen_stream(seed, (uint64_t)i);
    uint32_t k[GEN_MAX_DIM];
    for (int d = 0; d < GEN_MAX_DIM; ++d) k[d] = d < g.dim ? geo_coord(stream, d) : 0;
    for (int d = 0; d < g.dim; ++d) {
        coords[i * g.dim + d] = k[d];
        pos[i * g.dim + d] = (float)k[d] * (1.0f / 16777216.0f);
    }
    cell[i] = geo_cell(g, k);
    ids[i] = (uint32_t)i;
}

__global__ __launch_bounds__(GEN_BLOCK) void gen_geo_gather_kernel(int64_t n, int32_t dim, const uint32_t *__restrict__ coords,
                                                                  const uint32_t *__restrict__ sid, uint32_t *scoords) {
    const int64_t i = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t src = sid[i];
    for (int d = 0; d < dim; ++d) scoords[i * dim + d] = coords[src * dim + d];
}

// start[c] = the first sorted point whose cell is >= c, c = 0 .. n_cells (start[n_cells] = n)
__global__ __launch_bounds__(GEN_BLOCK) void gen_geo_cells_kernel(int64_t n, int64_t n_cells, const uint32_t *__restrict__ scell,
                                                                 int32_t *start) {
    const int64_t c = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (c > n_cells) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if ((int64_t)scell[mid] < c) lo = mid + 1; else hi = mid;
    }
    start[c] = (int32_t)lo;
}

// The pairs of sorted point i with a larger original id.  emit(key, index among i's pairs).
template <class Emit>
__host__ __device__ __forceinline__ int64_t geo_pairs(int64_t i, const GeoGrid &g, const uint32_t *scoords, const uint32_t *sid,
                                                       const int32_t *start, Emit emit) {
    uint32_t k[GEN_MAX_DIM];
    for (int d = 0; d < GEN_MAX_DIM; ++d) k[d] = d < g.dim ? scoords[i * g.dim + d] : 0;
    const int64_t u = sid[i];
    int32_t c[3] = {0, 0, 0};   // own cell per grid axis, axis gdim-1 is the contiguous one
    for (int d = 0; d < g.gdim; ++d) c[d] = (int32_t)(k[d] / g.side);
    const int32_t nc = (int32_t)g.ncell;
    const int last = g.gdim - 1;
    const int32_t l0 = c[last] > 0 ? c[last] - 1 : 0, l1 = c[last] + 1 < nc ? c[last] + 1 : nc - 1;
    const int r0 = g.gdim >= 2 ? 1 : 0, r1 = g.gdim >= 3 ? 1 : 0;   // reach along the outer axes
    int64_t count = 0;
    for (int d0 = -r0; d0 <= r0; ++d0) {
        for (int d1 = -r1; d1 <= r1; ++d1) {
            int64_t base = 0;
            if (g.gdim >= 2) {
                const int32_t a0 = c[0] + d0;
                if (a0 < 0 || a0 >= nc) continue;
                base = a0;
            }
            if (g.gdim >= 3) {
                const int32_t a1 = c[1] + d1;
                if (a1 < 0 || a1 >= nc) continue;
                base = base * nc + a1;
            }
            base *= nc;
            const int32_t jb = start[base + l0], je = start[base + l1 + 1];
            for (int32_t j = jb; j < je; ++j) {
                const int64_t v = sid[j];
                if (v <= u) continue;
                uint64_t d2 = 0;
                for (int d = 0; d < g.dim; ++d) {
                    const int64_t diff = (int64_t)k[d] - (int64_t)scoords[(int64_t)j * g.dim + d];
                    d2 += (uint64_t)(diff * diff);
                }
                if (d2 <= g.R2) { emit(((uint64_t)u << 32) | (uint64_t)v, count); ++count; }
            }
        }
    }
    return count;
}

template <bool WRITE>
__global__ __launch_bounds__(GEN_BLOCK) void gen_geo_pairs_kernel(int64_t n, GeoGrid g, const uint32_t *__restrict__ scoords,
                                                                 const uint32_t *__restrict__ sid, const int32_t *__restrict__ start,
                                                                 int64_t *counts, const int64_t *__restrict__ offsets, uint64_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (WRITE) geo_pairs(i, g, scoords, sid, start, EmitAt{keys + offsets[i]});
    else counts[i] = geo_pairs(i, g, scoords, sid, start, EmitNone{});
}

// ---- preferential attachment ----------------------------------------------------------------------------------------
// State per vertex v > m: tgt[v * m + t] the accepted targets, acc[v] how many, att[v] the next attempt, done[v] the round
// it finished in (INT32_MAX until then).  Continues v in round `round`; returns true when v holds m targets.  A slot of a
// vertex that did not finish before this round stops v at that attempt.
__host__ __device__ __forceinline__ bool ba_advance(int64_t v, int64_t m, uint64_t seed, int32_t round, int32_t *tgt, int32_t *acc,
                                                     int64_t *att, const int32_t *done) {
    const uint64_t stream = gen_stream(seed, (uint64_t)v);
    const uint64_t len = 2 * (uint64_t)m * (uint64_t)(v - m);
    int32_t *mine = tgt + v * m;
    int32_t t = acc[v];
    int64_t a = att[v];
    bool finished = true;
    while (t < m) {
        const uint64_t s = gen_mulhi(gen_word(stream, (uint64_t)a), len);
        int32_t x;
        if (s < 2 * (uint64_t)m) x = (s & 1) ? (int32_t)((s + 1) / 2) : 0;
        else {
            const int64_t w = m + (int64_t)(s / (2 * (uint64_t)m));
            if (!(s & 1)) x = (int32_t)w;
            else {
                if (done[w] >= round) { finished = false; break; }
                x = tgt[w * m + (int64_t)((s % (2 * (uint64_t)m)) / 2)];
            }
        }
        ++a;
        bool held = false;
        for (int32_t q = 0; q < t; ++q) held |= mine[q] == x;
        if (!held) mine[t++] = x;
    }
    acc[v] = t;
    att[v] = a;
    return finished;
}

__global__ __launch_bounds__(GEN_BLOCK) void gen_ba_init_kernel(int64_t n, int64_t m, int32_t *acc, int64_t *att, int32_t *done,
                                                               int32_t *list) {
    const int64_t v = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (v >= n) return;
    acc[v] = 0;
    att[v] = 0;
    done[v] = v <= m ? 0 : INT32_MAX;
    if (v > m) list[v - m - 1] = (int32_t)v;
}

__global__ __launch_bounds__(GEN_BLOCK) void gen_ba_round_kernel(int64_t n_active, const int32_t *__restrict__ cur, int32_t *nxt,
                                                                int32_t *nxt_count, int64_t m, uint64_t seed, int32_t round,
                                                                int32_t *tgt, int32_t *acc, int64_t *att, int32_t *done) {
    const int64_t i = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (i >= n_active) return;
    const int64_t v = cur[i];
    if (ba_advance(v, m, seed, round, tgt, acc, att, done)) done[v] = round;
    else nxt[atomicAdd(nxt_count, 1)] = (int32_t)v;
}

__global__ __launch_bounds__(GEN_BLOCK) void gen_ba_keys_kernel(int64_t n, int64_t m, const int32_t *__restrict__ tgt, uint64_t *keys) {
    const int64_t e = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;   // edge e: star first, then m per vertex
    if (e >= m * (n - m)) return;
    if (e < m) { keys[e] = (uint64_t)(e + 1); return; }
    const int64_t v = m + 1 + (e - m) / m, t = (e - m) % m;
    keys[e] = ((uint64_t)tgt[v * m + t] << 32) | (uint64_t)v;
}

__global__ __launch_bounds__(GEN_BLOCK) void gen_unpack_kernel(int64_t n_edges, const uint64_t *__restrict__ keys, int32_t *edges) {
    const int64_t e = (int64_t)blockIdx.x * GEN_BLOCK + threadIdx.x;
    if (e >= n_edges) return;
    const uint64_t k = keys[e];
    edges[2 * e] = (int32_t)(k >> 32);
    edges[2 * e + 1] = (int32_t)(k & 0xFFFFFFFFu);
}

inline unsigned gen_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + GEN_BLOCK - 1) / GEN_BLOCK); }
inline int gen_bits(int64_t n) { int b = 1; while (b < 32 && ((int64_t)1 << b) < n) ++b; return b; }

}  // namespace

struct gh_gen : gh_host {           // device < 0: host path
    int64_t n_edges = 0;
    gh_dev<int32_t> d_edges;         // device result (E, 2)
    std::vector<int32_t> h_edges;    // host-path result
    int64_t pos_count = 0;           // n * dim of the last geometric call
    gh_dev<float> d_pos;
    std::vector<float> h_pos;
};

static thread_local std::string g_gen_error;

namespace {

void gen_drop_result(gh_gen *h) {
    h->d_edges.reset();
    h->d_pos.reset();
    h->h_edges.clear();
    h->h_pos.clear();
    h->n_edges = 0;
    h->pos_count = 0;
}

gh_status gen_over_budget(gh_gen *h, const char *what, int64_t edges, int64_t bytes) {
    h->err = std::string(what) + ": " + (edges >= 0 ? std::to_string(edges) + " edges need " : "needs ") + std::to_string(bytes) +
             " bytes, the memory budget is " + std::to_string(h->budget);
    return GH_ERR_NOMEM;
}

// Sorts `keys` (n_edges of them, device) with `alt` as the second buffer and leaves the int32 pairs in h->d_edges.
gh_status gen_finish_device(gh_gen *h, gh_dev<uint64_t> &keys, gh_dev<uint64_t> &alt, int64_t n_edges, int64_t n_vertices) {
    if (n_edges >= ((int64_t)1 << 31)) { h->err = "more than 2^31 - 1 edges"; return GH_ERR_INVALID; }
    if (n_edges > 0) {
        hipcub::DoubleBuffer<uint64_t> db(keys.p, alt.p);
        size_t temp = 0;
        const int end_bit = 32 + gen_bits(n_vertices);
        GH_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, temp, db, (int)n_edges, 0, end_bit, h->stream));
        gh_dev<void> tmp;
        if (!tmp.alloc(temp)) { h->err = "hipMalloc failed for the sort's work space"; return GH_ERR_NOMEM; }
        GH_HIP(hipcub::DeviceRadixSort::SortKeys(tmp.p, temp, db, (int)n_edges, 0, end_bit, h->stream));
        // the pairs go into whichever buffer the sorted keys are not in: 8 bytes per edge either way
        gh_dev<uint64_t> &out = db.Current() == keys.p ? alt : keys;
        gen_unpack_kernel<<<dim3(gen_grid(n_edges)), dim3(GEN_BLOCK), 0, h->stream>>>(n_edges, db.Current(), out.as<int32_t>());
        GH_HIP(hipGetLastError());
        GH_HIP(hipStreamSynchronize(h->stream));
        h->d_edges = std::move(out);
    }
    h->n_edges = n_edges;
    return GH_OK;
}

void gen_finish_host(gh_gen *h, std::vector<uint64_t> &keys) {
    std::sort(keys.begin(), keys.end());
    h->h_edges.resize(2 * keys.size());
    for (size_t e = 0; e < keys.size(); ++e) {
        h->h_edges[2 * e] = (int32_t)(keys[e] >> 32);
        h->h_edges[2 * e + 1] = (int32_t)(keys[e] & 0xFFFFFFFFu);
    }
    h->n_edges = (int64_t)keys.size();
}

// counts (device int64[items]) -> exclusive offsets in place of `offsets`; total through the host.
gh_status gen_scan(gh_gen *h, const int64_t *counts, int64_t *offsets, int64_t items, int64_t *total) {
    *total = 0;
    if (items == 0) return GH_OK;
    if (items >= ((int64_t)1 << 31)) { h->err = "more than 2^31 - 1 work items"; return GH_ERR_INVALID; }
    size_t temp = 0;
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, counts, offsets, (int)items, h->stream));
    gh_dev<void> tmp;
    if (!tmp.alloc(temp)) { h->err = "hipMalloc failed for the scan's work space"; return GH_ERR_NOMEM; }
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, temp, counts, offsets, (int)items, h->stream));
    int64_t last_off = 0, last_cnt = 0;
    GH_HIP(hipMemcpyAsync(&last_off, offsets + items - 1, 8, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(&last_cnt, counts + items - 1, 8, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    *total = last_off + last_cnt;
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_gen_create(gh_gen_handle *out, int device_id) {
    if (!out) { g_gen_error = "out is NULL"; return GH_ERR_INVALID; }
    *out = nullptr;
    gh_gen *h = new gh_gen();
    h->budget = GEN_DEFAULT_BUDGET;
    if (device_id >= 0) {
        const gh_status st = gh_host_open(h, device_id, &g_gen_error);
        if (st != GH_OK) { gh_gen_destroy(h); return st; }
    }
    *out = h;
    return GH_OK;
}

extern "C" void gh_gen_destroy(gh_gen_handle h) {
    if (!h) return;
    gh_host_close(h);
    delete h;
}

extern "C" const char *gh_gen_last_error(gh_gen_handle h) { return h ? h->err.c_str() : g_gen_error.c_str(); }

extern "C" gh_status gh_gen_set_memory_budget(gh_gen_handle h, int64_t bytes) {
    return gh_host_set_budget(h, bytes, GEN_DEFAULT_BUDGET, &g_gen_error);
}

extern "C" gh_status gh_gen_sbm(gh_gen_handle h, int32_t n_blocks, const int64_t *sizes, const double *P, uint64_t seed,
                                int64_t *n_edges) {
    if (!h) { g_gen_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (!n_edges) return fail(GH_ERR_INVALID, "n_edges is NULL");
    *n_edges = 0;
    if (n_blocks < 0 || n_blocks > 4096 || (n_blocks > 0 && (!sizes || !P))) return fail(GH_ERR_INVALID, "n_blocks must be in [0, 4096]");
    const int64_t B = n_blocks;
    std::vector<int64_t> off((size_t)B + 1, 0);
    for (int64_t a = 0; a < B; ++a) {
        if (sizes[a] < 0) return fail(GH_ERR_INVALID, "block sizes must be >= 0");
        off[a + 1] = off[a] + sizes[a];
        if (off[a + 1] >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "more than 2^31 - 1 vertices");
    }
    for (int64_t a = 0; a < B; ++a)
        for (int64_t b = 0; b < B; ++b) {
            const double p = P[a * B + b];
            if (!(p >= 0.0 && p <= 1.0)) return fail(GH_ERR_INVALID, "probabilities must be in [0, 1]");
            if (p != P[b * B + a]) return fail(GH_ERR_INVALID, "the probability matrix must be symmetric");
        }
    // block pairs, segments, one gap table per distinct probability
    std::vector<SbmPair> pairs;
    std::vector<double> probs;
    std::vector<uint64_t> tables;
    int64_t n_seg = 0;
    for (int64_t a = 0; a < B; ++a)
        for (int64_t b = a; b < B; ++b) {
            SbmPair bp{};
            bp.seg0 = n_seg;
            bp.off_a = off[a]; bp.off_b = off[b]; bp.s_a = sizes[a]; bp.s_b = sizes[b];
            bp.diag = a == b;
            bp.N = a == b ? sizes[a] * (sizes[a] - 1) / 2 : sizes[a] * sizes[b];
            const double p = P[a * B + b];
            bp.table = -1;
            if (p > 0.0 && bp.N > 0) {
                size_t t = std::find(probs.begin(), probs.end(), p) - probs.begin();
                if (t == probs.size()) {
                    probs.push_back(p);
                    const double q = 1.0 - p;
                    double pw = 1.0;
                    for (int k = 0; k < GEN_TAB; ++k) {
                        pw = pw * q;
                        tables.push_back((uint64_t)std::floor((1.0 - pw) * 4503599627370496.0));
                    }
                }
                bp.table = (int32_t)t;
            }
            n_seg += (bp.N + GEN_SEG - 1) / GEN_SEG;
            pairs.push_back(bp);
        }
    if (h->device >= 0) (void)hipSetDevice(h->device);
    gen_drop_result(h);
    const int64_t n_pairs = (int64_t)pairs.size();
    if (n_seg == 0) return GH_OK;

    if (h->device < 0) {
        std::vector<uint64_t> keys;
        for (int64_t g = 0; g < n_seg; ++g)
            sbm_walk(g, seed, pairs.data(), n_pairs, tables.data(), [&](uint64_t key, int64_t) { keys.push_back(key); });
        gen_finish_host(h, keys);
        *n_edges = h->n_edges;
        return GH_OK;
    }
    if (16 * n_seg > h->budget) return gen_over_budget(h, "block model segment counts", -1, 16 * n_seg);
    gh_dev<SbmPair> d_pairs;
    gh_dev<uint64_t> d_tables, d_keys, d_alt;
    gh_dev<int64_t> d_counts, d_offsets;
    if (!d_pairs.alloc(sizeof(SbmPair) * pairs.size()) || !d_tables.alloc(8 * tables.size()) || !d_counts.alloc(8 * n_seg) ||
        !d_offsets.alloc(8 * n_seg))
        return fail(GH_ERR_NOMEM, "hipMalloc failed for the block model's segment state");
    GH_HIP(hipMemcpyAsync(d_pairs.p, pairs.data(), sizeof(SbmPair) * pairs.size(), hipMemcpyHostToDevice, h->stream));
    if (!tables.empty()) GH_HIP(hipMemcpyAsync(d_tables.p, tables.data(), 8 * tables.size(), hipMemcpyHostToDevice, h->stream));
    const unsigned grid = std::min<unsigned>(gen_grid(n_seg), GEN_MAX_BLOCKS);
    gen_sbm_kernel<false><<<dim3(grid), dim3(GEN_BLOCK), 0, h->stream>>>(n_seg, seed, d_pairs.p, n_pairs, d_tables.p,
                                                                       d_counts.p, nullptr, nullptr);
    GH_HIP(hipGetLastError());
    int64_t total = 0;
    gh_status st = gen_scan(h, d_counts.p, d_offsets.p, n_seg, &total);
    if (st != GH_OK) return st;
    if (16 * n_seg + 16 * total > h->budget) return gen_over_budget(h, "block model", total, 16 * n_seg + 16 * total);
    if (!d_keys.alloc(8 * total) || !d_alt.alloc(8 * total)) return fail(GH_ERR_NOMEM, "hipMalloc failed for " + std::to_string(total) + " edges");
    gen_sbm_kernel<true><<<dim3(grid), dim3(GEN_BLOCK), 0, h->stream>>>(n_seg, seed, d_pairs.p, n_pairs, d_tables.p,
                                                                      nullptr, d_offsets.p, d_keys.p);
    GH_HIP(hipGetLastError());
    st = gen_finish_device(h, d_keys, d_alt, total, off[B]);
    if (st != GH_OK) return st;
    *n_edges = total;
    return GH_OK;
}

extern "C" gh_status gh_gen_geometric(gh_gen_handle h, int64_t n, double radius, int32_t dim, uint64_t seed, int64_t *n_edges) {
    if (!h) { g_gen_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (!n_edges) return fail(GH_ERR_INVALID, "n_edges is NULL");
    *n_edges = 0;
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "n must be in [0, 2^31)");
    if (dim < 1 || dim > GEN_MAX_DIM) return fail(GH_ERR_INVALID, "dim must be in [1, 8]");
    if (!(radius >= 0.0)) return fail(GH_ERR_INVALID, "radius must be >= 0");
    GeoGrid g{};
    g.dim = dim;
    g.gdim = std::min(dim, 3);
    g.R2 = (uint64_t)std::floor(std::min(radius * radius, 16.0) * 281474976710656.0);
    // cell side >= the largest coordinate difference an edge can have (floor(sqrt(R2)), made exact in integers), and few
    // enough cells per axis that the table stays within about 4 n entries
    uint64_t rr = (uint64_t)std::sqrt((double)g.R2);
    while (rr * rr > g.R2) --rr;
    while ((rr + 1) * (rr + 1) <= g.R2) ++rr;
    uint64_t cmax = 1;
    while (cmax < (1ull << (30 / g.gdim)) && std::pow((double)(cmax + 1), g.gdim) <= 4.0 * (double)std::max<int64_t>(n, 1)) ++cmax;
    const uint64_t side = std::min<uint64_t>(GEN_COORD_ONE, std::max<uint64_t>({rr, 1, (GEN_COORD_ONE + cmax - 1) / cmax}));
    g.side = (uint32_t)side;
    g.ncell = (uint32_t)((GEN_COORD_ONE - 1) / side + 1);
    int64_t n_cells = 1;
    for (int d = 0; d < g.gdim; ++d) n_cells *= g.ncell;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    gen_drop_result(h);
    h->pos_count = n * dim;
    if (n == 0) return GH_OK;

    if (h->device < 0) {
        std::vector<uint32_t> coords((size_t)n * dim), scoords((size_t)n * dim), sid((size_t)n);
        std::vector<std::pair<uint32_t, uint32_t>> order((size_t)n);
        h->h_pos.resize((size_t)n * dim);
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t stream = gen_stream(seed, (uint64_t)i);
            uint32_t k[GEN_MAX_DIM] = {0};
            for (int d = 0; d < dim; ++d) {
                k[d] = coords[i * dim + d] = geo_coord(stream, d);
                h->h_pos[i * dim + d] = (float)k[d] * (1.0f / 16777216.0f);
            }
            order[i] = {geo_cell(g, k), (uint32_t)i};
        }
        std::sort(order.begin(), order.end());
        std::vector<int32_t> start((size_t)n_cells + 1, 0);
        for (int64_t i = 0; i < n; ++i) {
            sid[i] = order[i].second;
            for (int d = 0; d < dim; ++d) scoords[i * dim + d] = coords[(int64_t)sid[i] * dim + d];
            ++start[order[i].first + 1];
        }
        for (int64_t c = 0; c < n_cells; ++c) start[c + 1] += start[c];
        std::vector<uint64_t> keys;
        for (int64_t i = 0; i < n; ++i)
            geo_pairs(i, g, scoords.data(), sid.data(), start.data(), [&](uint64_t key, int64_t) { keys.push_back(key); });
        gen_finish_host(h, keys);
        *n_edges = h->n_edges;
        return GH_OK;
    }
    gh_dev<uint32_t> d_coords, d_scoords, d_cell, d_scell, d_ids, d_sid;
    gh_dev<int32_t> d_start;
    gh_dev<int64_t> d_counts, d_offsets;
    gh_dev<uint64_t> d_keys, d_alt;
    gh_dev<void> d_tmp;
    if (!h->d_pos.alloc(4 * (size_t)n * dim)) return fail(GH_ERR_NOMEM, "hipMalloc failed for the positions");
    if (!d_coords.alloc(4 * (size_t)n * dim) || !d_scoords.alloc(4 * (size_t)n * dim) || !d_cell.alloc(4 * n) || !d_scell.alloc(4 * n) ||
        !d_ids.alloc(4 * n) || !d_sid.alloc(4 * n) || !d_start.alloc(4 * (n_cells + 1)) || !d_counts.alloc(8 * n) || !d_offsets.alloc(8 * n))
        return fail(GH_ERR_NOMEM, "hipMalloc failed for the geometric graph's point state");
    const dim3 blk(GEN_BLOCK), grd(gen_grid(n));
    gen_geo_points_kernel<<<grd, blk, 0, h->stream>>>(n, seed, g, d_coords.p, h->d_pos.p, d_cell.p, d_ids.p);
    GH_HIP(hipGetLastError());
    size_t temp = 0;
    const int cell_bits = gen_bits(n_cells);
    GH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp, d_cell.p, d_scell.p, d_ids.p,
                                               d_sid.p, (int)n, 0, cell_bits, h->stream));
    if (!d_tmp.alloc(temp)) return fail(GH_ERR_NOMEM, "hipMalloc failed for the sort's work space");
    GH_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, temp, d_cell.p, d_scell.p, d_ids.p,
                                               d_sid.p, (int)n, 0, cell_bits, h->stream));
    gen_geo_gather_kernel<<<grd, blk, 0, h->stream>>>(n, dim, d_coords.p, d_sid.p, d_scoords.p);
    gen_geo_cells_kernel<<<dim3(gen_grid(n_cells + 1)), blk, 0, h->stream>>>(n, n_cells, d_scell.p, d_start.p);
    gen_geo_pairs_kernel<false><<<grd, blk, 0, h->stream>>>(n, g, d_scoords.p, d_sid.p, d_start.p, d_counts.p, nullptr, nullptr);
    GH_HIP(hipGetLastError());
    int64_t total = 0;
    gh_status st = gen_scan(h, d_counts.p, d_offsets.p, n, &total);
    if (st != GH_OK) return st;
    if (16 * total > h->budget) return gen_over_budget(h, "geometric graph", total, 16 * total);
    if (!d_keys.alloc(8 * total) || !d_alt.alloc(8 * total)) return fail(GH_ERR_NOMEM, "hipMalloc failed for " + std::to_string(total) + " edges");
    gen_geo_pairs_kernel<true><<<grd, blk, 0, h->stream>>>(n, g, d_scoords.p, d_sid.p, d_start.p, nullptr, d_offsets.p, d_keys.p);
    GH_HIP(hipGetLastError());
    st = gen_finish_device(h, d_keys, d_alt, total, n);
    if (st != GH_OK) return st;
    *n_edges = total;
    return GH_OK;
}

extern "C" gh_status gh_gen_ba(gh_gen_handle h, int64_t n, int64_t m, uint64_t seed, int64_t *n_edges, int32_t *rounds) {
    if (!h) { g_gen_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (!n_edges) return fail(GH_ERR_INVALID, "n_edges is NULL");
    *n_edges = 0;
    if (rounds) *rounds = 0;
    if (n >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "n must be below 2^31");
    if (m < 1 || m >= n) return fail(GH_ERR_INVALID, "m must satisfy 1 <= m < n");
    const int64_t E = m * (n - m);
    if (E >= ((int64_t)1 << 31) || n * m >= ((int64_t)1 << 40)) return fail(GH_ERR_INVALID, "more than 2^31 - 1 edges");
    if (h->device >= 0) (void)hipSetDevice(h->device);
    gen_drop_result(h);

    if (h->device < 0) {
        // in vertex order every slot drawn belongs to a finished vertex: one pass
        std::vector<int32_t> tgt((size_t)(n * m)), acc((size_t)n, 0), done((size_t)n, 0);
        std::vector<int64_t> att((size_t)n, 0);
        std::vector<uint64_t> keys;
        keys.reserve((size_t)E);
        for (int64_t i = 1; i <= m; ++i) keys.push_back((uint64_t)i);
        for (int64_t v = m + 1; v < n; ++v) {
            ba_advance(v, m, seed, 1, tgt.data(), acc.data(), att.data(), done.data());
            for (int64_t t = 0; t < m; ++t) keys.push_back(((uint64_t)tgt[v * m + t] << 32) | (uint64_t)v);
        }
        gen_finish_host(h, keys);
        *n_edges = h->n_edges;
        return GH_OK;
    }
    const int64_t state = n * m * 4 + n * (4 + 8 + 4 + 8);
    if (16 * E + state > h->budget) return gen_over_budget(h, "preferential attachment", E, 16 * E + state);
    gh_dev<int32_t> d_tgt, d_acc, d_done, d_list0, d_list1, d_cnt;
    gh_dev<int64_t> d_att;
    gh_dev<uint64_t> d_keys, d_alt;
    if (!d_tgt.alloc(4 * n * m) || !d_acc.alloc(4 * n) || !d_att.alloc(8 * n) || !d_done.alloc(4 * n) || !d_list0.alloc(4 * n) ||
        !d_list1.alloc(4 * n) || !d_cnt.alloc(4) || !d_keys.alloc(8 * E) || !d_alt.alloc(8 * E))
        return fail(GH_ERR_NOMEM, "hipMalloc failed for " + std::to_string(E) + " edges of attachment state");
    const dim3 blk(GEN_BLOCK);
    gen_ba_init_kernel<<<dim3(gen_grid(n)), blk, 0, h->stream>>>(n, m, d_acc.p, d_att.p, d_done.p, d_list0.p);
    GH_HIP(hipGetLastError());
    int64_t active = n - m - 1;
    int32_t round = 0;
    while (active > 0) {
        if (round >= GH_GEN_BA_MAX_ROUNDS)
            return fail(GH_ERR_RUNTIME, "preferential attachment: " + std::to_string(active) + " vertices unresolved after " +
                                            std::to_string(round) + " rounds");
        ++round;
        int32_t *cur = (round & 1) ? d_list0.p : d_list1.p;
        int32_t *nxt = (round & 1) ? d_list1.p : d_list0.p;
        GH_HIP(hipMemsetAsync(d_cnt.p, 0, 4, h->stream));
        gen_ba_round_kernel<<<dim3(gen_grid(active)), blk, 0, h->stream>>>(active, cur, nxt, d_cnt.p, m, seed, round,
                                                                          d_tgt.p, d_acc.p, d_att.p, d_done.p);
        GH_HIP(hipGetLastError());
        int32_t left = 0;
        GH_HIP(hipMemcpyAsync(&left, d_cnt.p, 4, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        if (left >= active)
            return fail(GH_ERR_RUNTIME, "preferential attachment: round " + std::to_string(round) + " finished no vertex");
        active = left;
    }
    if (rounds) *rounds = round;
    gen_ba_keys_kernel<<<dim3(gen_grid(E)), blk, 0, h->stream>>>(n, m, d_tgt.p, d_keys.p);
    GH_HIP(hipGetLastError());
    const gh_status st = gen_finish_device(h, d_keys, d_alt, E, n);
    if (st != GH_OK) return st;
    *n_edges = E;
    return GH_OK;
}

extern "C" gh_status gh_gen_edges(gh_gen_handle h, int32_t *edges) {
    if (!h) { g_gen_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->n_edges == 0) return GH_OK;
    if (!edges) { h->err = "edges is NULL"; return GH_ERR_INVALID; }
    if (h->device < 0) { std::copy(h->h_edges.begin(), h->h_edges.end(), edges); return GH_OK; }
    (void)hipSetDevice(h->device);
    GH_HIP(hipMemcpyAsync(edges, h->d_edges.p, 8 * (size_t)h->n_edges, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_gen_positions(gh_gen_handle h, float *positions) {
    if (!h) { g_gen_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->pos_count == 0) return GH_OK;
    if (!positions) { h->err = "positions is NULL"; return GH_ERR_INVALID; }
    if (h->device < 0) { std::copy(h->h_pos.begin(), h->h_pos.end(), positions); return GH_OK; }
    (void)hipSetDevice(h->device);
    GH_HIP(hipMemcpyAsync(positions, h->d_pos.p, 4 * (size_t)h->pos_count, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}
