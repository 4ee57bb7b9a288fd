// Link scores on the GPU (include/graphem_hip.h "link scores"; graphem-rapids_amd/links.py): the neighbourhood predictors
// of link prediction over the centrality handle's deduplicated symmetric CSR (neighbours ascending).  Every quantity on
// the device is an integer: counts, and fixed-point weights of scale 2^32 (W_ra by one integer division, W_aa from a table
// the host computes once per handle).  No result depends on the order of an atomic or on the number of workgroups.
//
// lk_pair_kernel        a group of G lanes (G = 4 .. 64, one value per launch) takes one pair: the lanes stride over the
//                       shorter row (gs_rows of csr_core.h picks it), each bisects the longer one, and xor-shuffles inside
//                       the group add up cn, aa and ra.
// lk_candidate_kernel   persistent workgroups take source rows off a ticket counter.  Each owns a slab of n 64-bit sums in
//                       global memory, zero on entry, and a buffer of n (id, value) entries; no word of either is touched
//                       by another workgroup.  Per source u:
//                         (a) groups of G lanes take the neighbours w of u, their lanes the neighbours v of w, and add the
//                             weight of deg w to slab[v];
//                         (b) the same walk exchanges slab[v] for 0.  The one lane that gets a non-zero value owns v, drops
//                             it when v = u or v is in row u, and appends (v, value) to the buffer through a counter in LDS.
//                             Every word that (a) touched is zero again: the slab is clean for the next source;
//                         (c) k passes over the buffer, each takes the best entry strictly below the one before under the
//                             total order (key by cross-multiplication, then the smaller id), so the passes need no marks.
//                       A hub source is served by one workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "cent_handle.h"
#include "csr_core.h"

#define LK_MAX_K 128
#define LK_MAX_DEGREE ((int64_t)1 << 30)
#define LK_MAX_WORKGROUPS 1024           // 4 workgroups of 256 threads on each of 256 CUs
#define LK_SLAB_BYTES 20                 // per vertex and workgroup: an 8-byte sum, a 4-byte id and an 8-byte value
#define LK_PAIR_BYTES 32                 // per pair: two ids and three sums
#define LK_ROW_ENTRIES ((int64_t)1 << 22)  // output entries (rows * k) of one candidate launch

namespace {

typedef unsigned long long lk_u64;

inline int64_t lk_w_ra(int64_t d) { return d > 0 ? (((int64_t)1 << 33) + d) / (2 * d) : 0; }
inline int64_t lk_w_aa(int64_t d) { return d >= 2 ? (int64_t)nearbyint(4294967296.0 / log((double)d)) : 0; }

__device__ __forceinline__ lk_u64 lk_dev_w_ra(int64_t d) { return d > 0 ? ((1ull << 33) + (lk_u64)d) / (2ull * (lk_u64)d) : 0ull; }

__global__ __launch_bounds__(GS_BLOCK) void lk_pair_kernel(int64_t n_pairs, int G, const int32_t *__restrict__ pairs,
                                                           const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                           const int64_t *__restrict__ w_aa, int64_t *cn, int64_t *aa, int64_t *ra) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t per_block = GS_BLOCK / G;
    for (int64_t p = (int64_t)blockIdx.x * per_block + threadIdx.x / G; p < n_pairs; p += (int64_t)gridDim.x * per_block) {
        const GsRows rows = gs_rows(ptr, pairs[2 * p], pairs[2 * p + 1]);
        int64_t c = 0, a = 0, r = 0;
        // the lanes stride over the short row and each bisects the whole long row: no window to carry, so not gs_common_walk
        for (int64_t k = rows.sb + lane; k < rows.se; k += G) {
            const int32_t w = adj[k];
            const int64_t at = gs_lower_bound(adj, rows.lb, rows.le, w);
            if (at < rows.le && adj[at] == w) {
                const int64_t d = ptr[w + 1] - ptr[w];
                c += 1;
                a += w_aa[d];
                r += (int64_t)lk_dev_w_ra(d);
            }
        }
        for (int off = G >> 1; off > 0; off >>= 1) {   // xor partners stay inside the aligned group of G lanes
            c += __shfl_xor(c, off);
            a += __shfl_xor(a, off);
            r += __shfl_xor(r, off);
        }
        if (lane == 0) { cn[p] = c; aa[p] = a; ra[p] = r; }
    }
}

// One candidate: id < 0 means none.
struct LkEntry {
    int32_t id;
    lk_u64 num, den;
};

// a ranks before b: the larger key, then the smaller id.  Both are candidates (id >= 0).
__device__ __forceinline__ bool lk_before(const LkEntry &a, const LkEntry &b) {
    const lk_u64 l = a.num * b.den, r = b.num * a.den;
    return l > r || (l == r && a.id < b.id);
}

__device__ __forceinline__ LkEntry lk_better(const LkEntry &a, const LkEntry &b) {
    if (b.id < 0) return a;
    if (a.id < 0) return b;
    return lk_before(a, b) ? a : b;
}

__global__ __launch_bounds__(GS_BLOCK) void lk_candidate_kernel(int32_t kind, int32_t k, int G, int64_t n, int64_t n_rows,
                                                                const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                                const int32_t *__restrict__ adj, const int64_t *__restrict__ w_aa,
                                                                lk_u64 *slabs, int32_t *buf_ids, lk_u64 *buf_vals, unsigned int *ticket,
                                                                int32_t *out_ids, int64_t *out_num, int64_t *out_den) {
    __shared__ unsigned int s_row, s_count;
    __shared__ LkEntry s_best[GS_BLOCK / 64];
    lk_u64 *slab = slabs + (int64_t)blockIdx.x * n;
    int32_t *bid = buf_ids + (int64_t)blockIdx.x * n;
    lk_u64 *bval = buf_vals + (int64_t)blockIdx.x * n;
    const int tid = threadIdx.x, lane = tid & (G - 1), group = tid / G, groups = GS_BLOCK / G;
    for (;;) {
        if (tid == 0) {
            s_row = atomicAdd(ticket, 1u);
            s_count = 0;
        }
        __syncthreads();
        const int64_t row = s_row;
        if (row >= n_rows) break;
        const int32_t u = rows[row];
        const int64_t ub = ptr[u], ue = ptr[u + 1];
        const lk_u64 deg_u = (lk_u64)(ue - ub);
        // (a) every wedge u - w - v adds the weight of deg w to slab[v]
        for (int64_t i = ub + group; i < ue; i += groups) {
            const int32_t w = adj[i];
            const int64_t wb = ptr[w], we = ptr[w + 1];
            const lk_u64 wt = kind == GH_LINK_AA ? (lk_u64)w_aa[we - wb] : kind == GH_LINK_RA ? lk_dev_w_ra(we - wb) : 1ull;
            if (wt == 0) continue;   // deg w = 1: w's only neighbour is u itself
            for (int64_t j = wb + lane; j < we; j += G) atomicAdd(&slab[adj[j]], wt);
        }
        // Slab and buffer are this workgroup's alone, so the barrier's workgroup-scope release / acquire is all the order
        // their words need.  A device-wide fence in front of each of the two barriers cost 30 of 50 ms on a 100 K-vertex
        // Barabasi-Albert graph (m = 5, k = 10, every vertex a source).
        __syncthreads();
        // (b) the lane that takes a non-zero sum out of slab[v] owns v
        for (int64_t i = ub + group; i < ue; i += groups) {
            const int32_t w = adj[i];
            const int64_t wb = ptr[w], we = ptr[w + 1];
            for (int64_t j = wb + lane; j < we; j += G) {
                const int32_t v = adj[j];
                const lk_u64 sum = atomicExch(&slab[v], 0ull);
                if (sum == 0 || v == u) continue;
                const int64_t at = gs_lower_bound(adj, ub, ue, v);
                if (at < ue && adj[at] == v) continue;
                const unsigned int slot = atomicAdd(&s_count, 1u);   // below n: v is a vertex, owned once
                bid[slot] = v;
                bval[slot] = kind == GH_LINK_PA ? deg_u * (lk_u64)(ptr[v + 1] - ptr[v]) : sum;
            }
        }
        __syncthreads();
        // (c) the k best of the buffer, best first
        const int64_t m = s_count;
        const int32_t found = (int32_t)(m < k ? m : k);
        LkEntry last{-1, 0, 1};
        for (int32_t r = 0; r < found; ++r) {
            LkEntry best{-1, 0, 1};
            for (int64_t i = tid; i < m; i += GS_BLOCK) {
                LkEntry e{bid[i], bval[i], 1};
                if (kind == GH_LINK_JACCARD) e.den = deg_u + (lk_u64)(ptr[e.id + 1] - ptr[e.id]) - e.num;
                if (last.id >= 0 && !lk_before(last, e)) continue;   // taken by an earlier pass
                best = lk_better(best, e);
            }
            for (int off = 32; off > 0; off >>= 1) {
                LkEntry o;
                o.id = __shfl_xor(best.id, off);
                o.num = __shfl_xor(best.num, off);
                o.den = __shfl_xor(best.den, off);
                best = lk_better(best, o);
            }
            if ((tid & 63) == 0) s_best[tid >> 6] = best;
            __syncthreads();
            last = s_best[0];
            for (int w = 1; w < GS_BLOCK / 64; ++w) last = lk_better(last, s_best[w]);
            if (tid == 0) {
                const int64_t o = row * k + r;
                out_ids[o] = last.id;
                out_num[o] = (int64_t)last.num;
                out_den[o] = (int64_t)last.den;
            }
            __syncthreads();
        }
        for (int32_t r = found + tid; r < k; r += GS_BLOCK) {
            const int64_t o = row * k + r;
            out_ids[o] = -1;
            out_num[o] = 0;
            out_den[o] = 1;
        }
        __syncthreads();   // s_row and s_count are rewritten at the top
    }
}

// Selects the device and, on the first link call of the handle, builds and uploads W_aa over 0 .. max_degree.
gh_status lk_prepare(gh_cent *h) {
    if (h->max_degree >= LK_MAX_DEGREE) {
        h->err = "link scores need a largest degree below 2^30, this graph has " + std::to_string(h->max_degree);
        return GH_ERR_INVALID;
    }
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    if (h->d_link_aa.p) return GH_OK;
    std::vector<int64_t> table((size_t)h->max_degree + 1);
    for (int64_t d = 0; d <= h->max_degree; ++d) table[(size_t)d] = lk_w_aa(d);
    gh_dev<int64_t> d_table;
    if (!d_table.alloc(8 * table.size())) { h->err = "hipMalloc failed for the weight table"; return GH_ERR_NOMEM; }
    GH_HIP(hipMemcpyAsync(d_table.p, table.data(), 8 * table.size(), hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    h->d_link_aa = std::move(d_table);
    return GH_OK;
}

// The lanes of a group: the power of two at or above the mean degree, 4 .. 64.
int lk_group_width(const gh_cent *h) {
    const int64_t mean = h->n ? (2 * h->edges + h->n - 1) / h->n : 0;
    int G = 4;
    while (G < 64 && G < mean) G <<= 1;
    return G;
}

// `items` pairs or rows of `width` ids each
gh_status lk_check_ids(gh_cent *h, int64_t items, int width, const int32_t *ids, const char *noun) {
    for (int64_t i = 0; i < items * width; ++i) {
        if (ids[i] < 0 || ids[i] >= h->n) {
            h->err = std::string(noun) + " " + std::to_string(i / width) + " has a vertex id outside [0, n)";
            return GH_ERR_INVALID;
        }
    }
    return GH_OK;
}

gh_status lk_scores(gh_cent *h, int64_t n_pairs, const int32_t *pairs, int64_t *cn, int64_t *aa, int64_t *ra) {
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_pairs, h->budget / LK_PAIR_BYTES));
    gh_dev<int32_t> d_pairs;
    gh_dev<int64_t> d_out;
    if (!d_pairs.alloc(8 * chunk) || !d_out.alloc(24 * chunk)) { h->err = "hipMalloc failed for the pair scores"; return GH_ERR_NOMEM; }
    const int G = lk_group_width(h);
    int64_t *outs[3] = {cn, aa, ra};
    for (int64_t lo = 0; lo < n_pairs; lo += chunk) {
        const int64_t cnt = std::min(chunk, n_pairs - lo);
        GH_HIP(hipMemcpyAsync(d_pairs.p, pairs + 2 * lo, 8 * cnt, hipMemcpyHostToDevice, h->stream));
        const int grid = gs_blocks(cnt * G);
        lk_pair_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(cnt, G, d_pairs.p, h->d_ptr.p, h->d_adj.p, h->d_link_aa.p, d_out.p,
                                                                    d_out.p + chunk, d_out.p + 2 * chunk);
        GH_HIP(hipGetLastError());
        for (int j = 0; j < 3; ++j)
            if (outs[j]) GH_HIP(hipMemcpyAsync(outs[j] + lo, d_out.p + j * chunk, 8 * cnt, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
    }
    return GH_OK;
}

gh_status lk_candidates(gh_cent *h, int32_t kind, int32_t k, int64_t n_rows, const int32_t *rows, int32_t *ids, int64_t *num, int64_t *den) {
    const int64_t n = h->n;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_rows, LK_ROW_ENTRIES / k));
    const int64_t groups = std::max<int64_t>(1, std::min<int64_t>({(int64_t)LK_MAX_WORKGROUPS, chunk, h->budget / (LK_SLAB_BYTES * n)}));
    gh_dev<lk_u64> d_slab, d_vals;
    gh_dev<int32_t> d_ids, d_rows, d_out_ids;
    gh_dev<int64_t> d_out;
    gh_dev<unsigned int> d_ticket;
    if (!d_slab.alloc(8 * n * groups) || !d_vals.alloc(8 * n * groups) || !d_ids.alloc(4 * n * groups) || !d_rows.alloc(4 * chunk) ||
        !d_out_ids.alloc(4 * chunk * k) || !d_out.alloc(16 * chunk * k) || !d_ticket.alloc(16)) {
        h->err = "hipMalloc failed for the link candidates";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemsetAsync(d_slab.p, 0, 8 * n * groups, h->stream));   // once: every source leaves its slab as it found it
    const int G = std::min(64, 4 * lk_group_width(h));   // the rows walked are neighbours' rows, longer than the mean row
    for (int64_t lo = 0; lo < n_rows; lo += chunk) {
        const int64_t cnt = std::min(chunk, n_rows - lo);
        GH_HIP(hipMemcpyAsync(d_rows.p, rows + lo, 4 * cnt, hipMemcpyHostToDevice, h->stream));
        GH_HIP(hipMemsetAsync(d_ticket.p, 0, 16, h->stream));
        lk_candidate_kernel<<<dim3((unsigned)std::min(groups, cnt)), dim3(GS_BLOCK), 0, h->stream>>>(
            kind, k, G, n, cnt, d_rows.p, h->d_ptr.p, h->d_adj.p, h->d_link_aa.p, d_slab.p, d_ids.p, d_vals.p, d_ticket.p, d_out_ids.p,
            d_out.p, d_out.p + chunk * k);
        GH_HIP(hipGetLastError());
        GH_HIP(hipMemcpyAsync(ids + lo * k, d_out_ids.p, 4 * cnt * k, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipMemcpyAsync(num + lo * k, d_out.p, 8 * cnt * k, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipMemcpyAsync(den + lo * k, d_out.p + chunk * k, 8 * cnt * k, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
    }
    return GH_OK;
}

}  // namespace

extern "C" int64_t gh_link_weight(int32_t kind, int64_t degree) {
    if (degree < 0 || degree >= LK_MAX_DEGREE) return -1;
    switch (kind) {
    case GH_LINK_AA: return lk_w_aa(degree);
    case GH_LINK_RA: return lk_w_ra(degree);
    case GH_LINK_CN: case GH_LINK_JACCARD: case GH_LINK_PA: return 1;
    default: return -1;
    }
}

extern "C" gh_status gh_cent_link_scores(gh_cent_handle h, int64_t n_pairs, const int32_t *pairs, int64_t *cn, int64_t *aa,
                                         int64_t *ra) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) { h->err = "bad pair list"; return GH_ERR_INVALID; }
    if (n_pairs == 0) return GH_OK;
    GH_TRY_ST(lk_check_ids(h, n_pairs, 2, pairs, "pair"));
    GH_TRY_ST(lk_prepare(h));
    const gh_status st = lk_scores(h, n_pairs, pairs, cn, aa, ra);
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    return st;
}

extern "C" gh_status gh_cent_link_candidates(gh_cent_handle h, int32_t kind, int32_t k, int64_t n_rows, const int32_t *rows,
                                             int32_t *ids, int64_t *num, int64_t *den) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (kind < GH_LINK_CN || kind > GH_LINK_PA) { h->err = "unknown score kind " + std::to_string(kind); return GH_ERR_INVALID; }
    if (k < 1 || k > LK_MAX_K) { h->err = "k must lie in [1, " + std::to_string(LK_MAX_K) + "]"; return GH_ERR_INVALID; }
    if (n_rows < 0 || (n_rows > 0 && (!rows || !ids || !num || !den))) { h->err = "bad row list or output"; return GH_ERR_INVALID; }
    if (n_rows == 0) return GH_OK;
    GH_TRY_ST(lk_check_ids(h, n_rows, 1, rows, "row"));
    GH_TRY_ST(lk_prepare(h));
    const gh_status st = lk_candidates(h, kind, k, n_rows, rows, ids, num, den);
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    return st;
}
