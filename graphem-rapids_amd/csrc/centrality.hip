// Centrality measures on the GPU (include/graphem_hip.h "centrality"; graphem-rapids_amd/centrality.py): shortest-path
// betweenness (Brandes), load (Newman) and closeness from one all-sources pass, PageRank, and the adjacency SpMV of the
// eigenvector solve.  Undirected, unweighted graphs; fp64 throughout, as networkx computes in Python floats.
//
// Paths.  A batch of B = 64 G sources; source j of the ordered list is lane j % 64 of group j / 64.  Per (vertex, source)
// entry the state is source-fastest, [group][vertex][lane], so the wave that owns (v, g) reads a neighbour's row of 64
// values as one contiguous 256 B (int32) or 512 B (double) load:
//     dist (int32, -1 = unreached), sigma (double, shortest paths), npred (int32, shortest-path predecessors),
//     delta (double, Brandes dependency), lam (double, Newman load dependency).
// Per (v, g) words: vis (uint64, lanes that reached v; invalid lanes of a short last group preset), cur / nxt (uint64, lanes
// whose BFS reached v at the previous / this level) and range (int2: first and last level any lane reached v at).
//
//   cent_init_kernel       dist, vis, cur, range of every (v, g); level-0 entries get sigma = 1.
//   cent_fwd_kernel (L)    pull: a wave per (v, g) with unreached lanes; lane s sums sigma over the neighbours u whose
//                          frontier word has bit s, counts them, and the lanes that found one set dist = L.  Writes its
//                          next frontier word (0 included), so the ping-pong buffers need no clearing; sets flag[L] when
//                          anything was reached.  A launch after the last level sees flag[L - 1] == 0 and returns.
//   cent_bwd_kernel (L)    deepest level first, pull: lane s of (x, g) with dist = L sums over neighbours w at L + 1
//                              delta[x] = sum sigma[x] * ((1 + delta[w]) / sigma[w])         (networkx _accumulate_basic)
//                              lam[x]   = sum (1 + lam[w]) / npred[w]                         (networkx load._node_betweenness)
//                          A neighbour's rows are loaded only when L + 1 lies in its level range.
//   cent_vertex_sum_kernel out[v] += lane-tree sum of the 64 lanes' delta / lam (lanes with dist >= 1: the source itself
//                          and unreached lanes add nothing), one group after the other in list order.
//   cent_source_sum_kernel reached / dist_sum per source: integer sums, so the order of the atomics cannot matter.
// Every (vertex, source) value is written by the one lane that owns it: no float atomics, and the result depends only on
// the graph and the ordered source list -- not on the batch width (budget), nor on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "cent_handle.h"

#define CENT_BLOCK 256
#define CENT_MAX_BLOCKS 4096
#define CENT_CHECK_EVERY 4            // forward levels between two host reads of the level flags
#define CENT_SRC_CHUNK 1024           // vertices per workgroup of the per-source sums
#define PR_BLOCK 256
#define PR_MAX_BLOCKS 2048
#define PR_CHECK_EVERY 8              // PageRank iterations between two host reads of the convergence flag

namespace {

struct CentLevel {
    const int64_t *ptr; const int32_t *adj;
    int32_t *dist, *npred;
    double *sigma, *delta, *lam;
    uint64_t *vis, *cur, *nxt;
    int2 *range;
    int32_t *flags;                 // flags[L] = 1: level L reached something
    int64_t n, G;
    int32_t level;
};

__device__ __forceinline__ int cent_lane() { return threadIdx.x & 63; }

// (v, g) items, a wave per item
#define CENT_WAVE_LOOP(items)                                                                                     \
    for (int64_t it = (int64_t)blockIdx.x * (CENT_BLOCK / 64) + (threadIdx.x >> 6); it < (items);                \
         it += (int64_t)gridDim.x * (CENT_BLOCK / 64))

__global__ __launch_bounds__(CENT_BLOCK) void cent_init_kernel(CentLevel a, const int32_t *__restrict__ sources, int64_t n_src) {
    const int lane = cent_lane();
    CENT_WAVE_LOOP(a.G * a.n) {
        const int64_t g = it / a.n, v = it - g * a.n;
        const int64_t j = g * 64 + lane;
        const bool valid = j < n_src;
        const bool src = valid && sources[j] == v;
        const int64_t e = it * 64 + lane;
        a.dist[e] = src ? 0 : -1;
        if (src) { a.sigma[e] = 1.0; a.npred[e] = 0; }
        const uint64_t s = __ballot(src), inv = __ballot(!valid);
        if (lane == 0) {
            a.vis[it] = s | inv;
            a.cur[it] = s;
            a.range[it] = s ? make_int2(0, 0) : make_int2(INT32_MAX, -1);
        }
    }
}

__global__ __launch_bounds__(CENT_BLOCK) void cent_fwd_kernel(CentLevel a) {
    if (__hip_atomic_load(&a.flags[a.level - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const int lane = cent_lane();
    CENT_WAVE_LOOP(a.G * a.n) {
        const int64_t g = it / a.n, v = it - g * a.n;
        const uint64_t need = ~a.vis[it];
        uint64_t found = 0;
        if (need) {
            const uint64_t *curg = a.cur + g * a.n;
            const double *sigg = a.sigma + g * a.n * 64;
            double sig = 0.0;
            int32_t np = 0;
            const int64_t beg = a.ptr[v], end = a.ptr[v + 1];
            for (int64_t k = beg; k < end; ++k) {
                const int32_t u = a.adj[k];
                const uint64_t f = curg[u] & need;
                if (f == 0) continue;
                if ((f >> lane) & 1) { sig += sigg[(int64_t)u * 64 + lane]; ++np; }
            }
            found = __ballot(np > 0);
            if (np > 0) {
                const int64_t e = it * 64 + lane;
                a.dist[e] = a.level;
                a.sigma[e] = sig;
                a.npred[e] = np;
            }
        }
        if (lane == 0) {
            a.nxt[it] = found;
            if (found) {
                a.vis[it] |= found;
                int2 r = a.range[it];
                r.x = min(r.x, a.level);
                r.y = a.level;
                a.range[it] = r;
                if (__hip_atomic_load(&a.flags[a.level], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) a.flags[a.level] = 1;
            }
        }
    }
}

__global__ __launch_bounds__(CENT_BLOCK) void cent_bwd_kernel(CentLevel a, int32_t want_delta, int32_t want_lam) {
    const int lane = cent_lane();
    const int32_t L = a.level;
    CENT_WAVE_LOOP(a.G * a.n) {
        const int2 r = a.range[it];
        if (L < r.x || L > r.y) continue;
        const int64_t g = it / a.n, v = it - g * a.n;
        const int64_t e = it * 64 + lane;
        const bool mine = a.dist[e] == L;
        if (__ballot(mine) == 0) continue;
        const double sx = mine ? a.sigma[e] : 0.0;
        double dacc = 0.0, lacc = 0.0;
        const int64_t beg = a.ptr[v], end = a.ptr[v + 1];
        for (int64_t k = beg; k < end; ++k) {
            const int64_t w = g * a.n + a.adj[k];
            const int2 rw = a.range[w];
            if (L + 1 < rw.x || L + 1 > rw.y) continue;
            const int64_t ew = w * 64 + lane;
            if (mine && a.dist[ew] == L + 1) {
                if (want_delta) dacc += sx * ((1.0 + a.delta[ew]) / a.sigma[ew]);
                if (want_lam) lacc += (1.0 + a.lam[ew]) / (double)a.npred[ew];
            }
        }
        if (mine) {
            if (want_delta) a.delta[e] = dacc;
            if (want_lam) a.lam[e] = lacc;
        }
    }
}

__device__ __forceinline__ double cent_wave_sum(double x) {   // fixed butterfly; lane 0's value is used
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__global__ __launch_bounds__(CENT_BLOCK) void cent_vertex_sum_kernel(CentLevel a, double *bc, double *ld) {
    const int lane = cent_lane();
    CENT_WAVE_LOOP(a.n) {
        const int64_t v = it;
        double sb = bc ? bc[v] : 0.0, sl = ld ? ld[v] : 0.0;
        for (int64_t g = 0; g < a.G; ++g) {
            const int64_t e = (g * a.n + v) * 64 + lane;
            const bool in = a.dist[e] >= 1;
            if (bc) { const double t = cent_wave_sum(in ? a.delta[e] : 0.0); sb += t; }
            if (ld) { const double t = cent_wave_sum(in ? a.lam[e] : 0.0); sl += t; }
        }
        if (lane == 0) {
            if (bc) bc[v] = sb;
            if (ld) ld[v] = sl;
        }
    }
}

// grid (chunks, G): lane s of every wave sums its source's reached count and distances over the chunk's vertices
__global__ __launch_bounds__(CENT_BLOCK) void cent_source_sum_kernel(CentLevel a, unsigned long long *reached,
                                                                    unsigned long long *dist_sum) {
    const int lane = cent_lane();
    const int64_t g = blockIdx.y;
    const int64_t v0 = (int64_t)blockIdx.x * CENT_SRC_CHUNK, v1 = min(a.n, v0 + CENT_SRC_CHUNK);
    unsigned long long cnt = 0, sum = 0;
    for (int64_t v = v0 + (threadIdx.x >> 6); v < v1; v += CENT_BLOCK / 64) {
        const int32_t d = a.dist[(g * a.n + v) * 64 + lane];
        if (d >= 0) { ++cnt; sum += (unsigned long long)d; }
    }
    if (cnt) {
        atomicAdd(&reached[g * 64 + lane], cnt);
        atomicAdd(&dist_sum[g * 64 + lane], sum);
    }
}

// ---- PageRank: networkx _pagerank_scipy on the device ---------------------------------------------------------------
struct PrState {
    double dsum;      // sum of x over the dangling vertices, of the current iterate
    int32_t done;     // 1 once converged or out of iterations
    int32_t iters;    // iteration that converged; -1: max_iter reached without
};

__device__ __forceinline__ double pr_block_sum(double v, double *red) {   // fixed order; thread 0 gets the sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    __syncthreads();
    return s;
}

// x0 = 1/N; partial sums of its dangling entries
__global__ __launch_bounds__(PR_BLOCK) void pr_init_kernel(int64_t n, const int64_t *__restrict__ ptr, double *x, double *dpart) {
    __shared__ double red[PR_BLOCK / 64];
    double d = 0.0;
    const double x0 = 1.0 / (double)n;
    for (int64_t i = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PR_BLOCK) {
        x[i] = x0;
        if (ptr[i + 1] == ptr[i]) d += x0;
    }
    const double s = pr_block_sum(d, red);
    if (threadIdx.x == 0) dpart[blockIdx.x] = s;
}

// y = alpha (x A_rownorm + dsum / N) + (1 - alpha) / N; 8 lanes per row; partial |y - x| and dangling sums per block
__global__ __launch_bounds__(PR_BLOCK) void pr_step_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                          const double *__restrict__ inv_deg, double alpha,
                                                          const PrState *st, const double *__restrict__ x, double *__restrict__ y,
                                                          double *epart, double *dpart) {
    __shared__ double red[PR_BLOCK / 64];
    if (st->done) return;
    const double pN = 1.0 / (double)n, dsum = st->dsum;
    const int sub = threadIdx.x & 7;
    double err = 0.0, dang = 0.0;
    const int64_t rows_per = (int64_t)gridDim.x * (PR_BLOCK / 8);
    const int64_t rounds = (n + rows_per - 1) / rows_per;
    for (int64_t q = 0; q < rounds; ++q) {   // every thread runs the same rounds (the shuffles need the whole wave)
        const int64_t row = q * rows_per + (int64_t)blockIdx.x * (PR_BLOCK / 8) + (threadIdx.x >> 3);
        int64_t beg = 0, end = 0;
        if (row < n) { beg = ptr[row]; end = ptr[row + 1]; }
        double acc = 0.0;
        for (int64_t j = beg + sub; j < end; j += 8) {
            const int32_t c = adj[j];
            acc += x[c] * inv_deg[c];
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (row < n && sub == 0) {
            const double yi = alpha * (acc + dsum * pN) + (1.0 - alpha) * pN;
            y[row] = yi;
            err += fabs(yi - x[row]);
            if (end == beg) dang += yi;
        }
    }
    const double se = pr_block_sum(err, red);
    const double sd = pr_block_sum(dang, red);
    if (threadIdx.x == 0) { epart[blockIdx.x] = se; dpart[blockIdx.x] = sd; }
}

// one workgroup: the L1 change and the next dangling sum; the convergence test of iteration `iter` (0: the start vector)
__global__ __launch_bounds__(PR_BLOCK) void pr_check_kernel(int32_t nparts, const double *epart, const double *dpart, double ntol,
                                                           int32_t iter, int32_t max_iter, PrState *st) {
    __shared__ double red[PR_BLOCK / 64];
    if (st->done) return;
    double e = 0.0, d = 0.0;
    for (int i = threadIdx.x; i < nparts; i += PR_BLOCK) {
        if (iter > 0) e += epart[i];
        d += dpart[i];
    }
    const double se = pr_block_sum(e, red);
    const double sd = pr_block_sum(d, red);
    if (threadIdx.x == 0) {
        st->dsum = sd;
        if (iter > 0 && se < ntol) { st->done = 1; st->iters = iter; }
        else if (iter >= max_iter) { st->done = 1; st->iters = -1; }
    }
}

// y = A x + c x, A the 0/1 adjacency; 8 lanes per row
__global__ __launch_bounds__(256) void spmv_adj_shift_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                            double c, const double *__restrict__ x, double *__restrict__ y) {
    const int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    double acc = 0.0;
    int64_t beg = 0, end = 0;
    if (row < n) { beg = ptr[row]; end = ptr[row + 1]; }
    for (int64_t j = beg + sub; j < end; j += 8) acc += x[adj[j]];
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (row < n && sub == 0) y[row] = acc + c * x[row];
}

inline int cent_blocks(int64_t waves) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(CENT_MAX_BLOCKS, (waves + CENT_BLOCK / 64 - 1) / (CENT_BLOCK / 64)));
}

}  // namespace

static thread_local std::string g_cent_error;
void cent_set_create_error(const std::string &msg) { g_cent_error = msg; }

namespace {

void cent_free_state(gh_cent *h) {
    h->d_dist.reset(); h->d_npred.reset(); h->d_flags.reset(); h->d_src.reset();
    h->d_sigma.reset(); h->d_delta.reset(); h->d_lam.reset();
    h->d_vis.reset(); h->d_fa.reset(); h->d_fb.reset(); h->d_range.reset();
    h->cap_groups = 0;
}

// device bytes of path state per 64-source group (the budget counts these)
int64_t cent_bytes_per_group(int64_t n) { return n * (64 * (4 + 8 + 4 + 8 + 8) + 3 * 8 + 8); }

gh_status cent_reserve(gh_cent *h, int64_t G) {
    if (G <= h->cap_groups) return GH_OK;
    cent_free_state(h);
    const int64_t ent = G * h->n * 64, words = G * h->n;
    if (!h->d_dist.alloc(4 * ent) || !h->d_npred.alloc(4 * ent) || !h->d_sigma.alloc(8 * ent) || !h->d_delta.alloc(8 * ent) ||
        !h->d_lam.alloc(8 * ent) || !h->d_vis.alloc(8 * words) || !h->d_fa.alloc(8 * words) || !h->d_fb.alloc(8 * words) ||
        !h->d_range.alloc(8 * words) || !h->d_flags.alloc(4 * (h->n + 2)) || !h->d_src.alloc(4 * 64 * G)) {
        cent_free_state(h);
        h->err = "hipMalloc failed for " + std::to_string(G) + " source groups of path state";
        return GH_ERR_NOMEM;
    }
    h->cap_groups = G;
    return GH_OK;
}

// One batch of ns <= 64 G sources: forward levels, backward levels, sums into the device outputs.
gh_status cent_run_batch(gh_cent *h, int64_t G, const int32_t *src, int64_t ns, double *d_bc, double *d_ld,
                         unsigned long long *d_reached, unsigned long long *d_dsum) {
    const int64_t n = h->n;
    CentLevel a{};
    a.ptr = h->d_ptr.p; a.adj = h->d_adj.p;
    a.dist = h->d_dist.p; a.npred = h->d_npred.p; a.sigma = h->d_sigma.p; a.delta = h->d_delta.p; a.lam = h->d_lam.p;
    a.vis = h->d_vis.p; a.range = h->d_range.p; a.flags = h->d_flags.p;
    a.n = n; a.G = G;
    GH_HIP(hipMemcpyAsync(h->d_src.p, src, 4 * ns, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemsetAsync(h->d_flags.p, 0, 4 * (n + 2), h->stream));
    const int32_t one = 1;
    GH_HIP(hipMemcpyAsync(h->d_flags.p, &one, 4, hipMemcpyHostToDevice, h->stream));
    const int grid = cent_blocks(G * n);
    a.cur = h->d_fa.p;
    cent_init_kernel<<<dim3(grid), dim3(CENT_BLOCK), 0, h->stream>>>(a, h->d_src.p, ns);
    GH_HIP(hipGetLastError());
    int32_t maxd = 0;
    GH_TRY_ST(gh_level_loop(h, n, h->d_flags.p, CENT_CHECK_EVERY, &maxd, [&](int32_t L) -> gh_status {
        a.level = L;
        a.cur = (L & 1) ? h->d_fa.p : h->d_fb.p;
        a.nxt = (L & 1) ? h->d_fb.p : h->d_fa.p;
        cent_fwd_kernel<<<dim3(grid), dim3(CENT_BLOCK), 0, h->stream>>>(a);
        GH_HIP(hipGetLastError());
        return GH_OK;
    }));
    const int want_delta = d_bc != nullptr, want_lam = d_ld != nullptr;
    if (want_delta || want_lam) {
        for (int32_t L = maxd; L >= 1; --L) {
            a.level = L;
            cent_bwd_kernel<<<dim3(grid), dim3(CENT_BLOCK), 0, h->stream>>>(a, want_delta, want_lam);
        }
        cent_vertex_sum_kernel<<<dim3(cent_blocks(n)), dim3(CENT_BLOCK), 0, h->stream>>>(a, d_bc, d_ld);
        GH_HIP(hipGetLastError());
    }
    if (d_reached) {
        cent_source_sum_kernel<<<dim3((unsigned)((n + CENT_SRC_CHUNK - 1) / CENT_SRC_CHUNK), (unsigned)G), dim3(CENT_BLOCK), 0,
                                 h->stream>>>(a, d_reached, d_dsum);
        GH_HIP(hipGetLastError());
    }
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_cent_create(gh_cent_handle *out, int device_id, int64_t n, int64_t n_edges, const int32_t *edges) {
    auto fail = [&](gh_status st, const std::string &msg) { g_cent_error = msg; return st; };
    if (!out) return fail(GH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "n must be in [1, 2^31)");
    if (n_edges < 0 || (n_edges > 0 && !edges)) return fail(GH_ERR_INVALID, "bad edge list");
    std::vector<uint64_t> key;
    GH_TRY_ST(gh_canonical_edge_keys(n, n_edges, edges, false, "edge", &key, &g_cent_error));
    std::vector<int64_t> ptr;
    std::vector<int32_t> adj;
    gh_csr_from_keys(n, key, GH_CSR_SYMMETRIC, &ptr, &adj);   // neighbours ascending
    std::vector<double> inv_deg((size_t)n);
    int64_t max_degree = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t d = ptr[i + 1] - ptr[i];
        inv_deg[i] = d ? 1.0 / (double)d : 0.0;
        max_degree = std::max(max_degree, d);
    }
    gh_cent *h = new gh_cent();
    h->budget = CENT_DEFAULT_BUDGET;
    h->n = n;
    h->edges = (int64_t)key.size();
    h->max_degree = max_degree;
    auto bail = [&](gh_status st, const std::string &msg) { gh_cent_destroy(h); return fail(st, msg); };
    const gh_status st = gh_host_open(h, device_id, &g_cent_error);
    if (st != GH_OK) { gh_cent_destroy(h); return st; }
    if (!h->d_ptr.alloc(8 * ptr.size()) || !h->d_adj.alloc(4 * adj.size()) || !h->d_inv_deg.alloc(8 * inv_deg.size()))
        return bail(GH_ERR_NOMEM, "hipMalloc failed");
    if (hipMemcpy(h->d_ptr.p, ptr.data(), 8 * ptr.size(), hipMemcpyHostToDevice) != hipSuccess ||
        (!adj.empty() && hipMemcpy(h->d_adj.p, adj.data(), 4 * adj.size(), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(h->d_inv_deg.p, inv_deg.data(), 8 * inv_deg.size(), hipMemcpyHostToDevice) != hipSuccess)
        return bail(GH_ERR_HIP, "upload failed");
    *out = h;
    return GH_OK;
}

extern "C" void gh_cent_destroy(gh_cent_handle h) {
    if (!h) return;
    gh_host_close(h);
    delete h;
}

extern "C" const char *gh_cent_last_error(gh_cent_handle h) { return h ? h->err.c_str() : g_cent_error.c_str(); }

extern "C" int64_t gh_cent_edge_count(gh_cent_handle h) { return h ? h->edges : -1; }

extern "C" gh_status gh_cent_csr_device(gh_cent_handle h, const int64_t **indptr, const int32_t **indices) {
    if (!h) g_cent_error = "handle is NULL";
    if (!h || !indptr || !indices) return GH_ERR_INVALID;
    *indptr = h->d_ptr.p;
    *indices = h->d_adj.p;
    return GH_OK;
}

extern "C" gh_status gh_cent_set_memory_budget(gh_cent_handle h, int64_t bytes) {
    return gh_host_set_budget(h, bytes, CENT_DEFAULT_BUDGET, &g_cent_error);
}

extern "C" gh_status gh_cent_paths(gh_cent_handle h, int64_t n_sources, const int32_t *sources, double *betweenness,
                                   double *load, int64_t *reached, int64_t *dist_sum) {
    if (!h) { g_cent_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (n_sources < 0 || (n_sources > 0 && !sources)) return fail(GH_ERR_INVALID, "bad source list");
    if ((reached == nullptr) != (dist_sum == nullptr)) return fail(GH_ERR_INVALID, "reached and dist_sum go together");
    for (int64_t i = 0; i < n_sources; ++i)
        if (sources[i] < 0 || sources[i] >= h->n) return fail(GH_ERR_INVALID, "source id outside [0, n)");
    const int64_t n = h->n;
    if (betweenness) std::fill(betweenness, betweenness + n, 0.0);
    if (load) std::fill(load, load + n, 0.0);
    if (reached) { std::fill(reached, reached + n_sources, (int64_t)0); std::fill(dist_sum, dist_sum + n_sources, (int64_t)0); }
    if (n_sources == 0 || (!betweenness && !load && !reached)) return GH_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    const int64_t groups = (n_sources + 63) / 64;
    int64_t G = std::max<int64_t>(1, h->budget / cent_bytes_per_group(n));
    G = std::min<int64_t>({G, groups, (int64_t)65535});   // 65535: grid.y of the per-source sums
    GH_TRY_ST(cent_reserve(h, G));
    gh_dev<double> d_bc, d_ld;               // allocated only for the outputs asked for
    gh_dev<unsigned long long> d_cnt;        // reached, then dist_sum, 64 per group
    if ((betweenness && !d_bc.alloc(8 * n)) || (load && !d_ld.alloc(8 * n)) || (reached && !d_cnt.alloc(16 * groups * 64)))
        return fail(GH_ERR_NOMEM, "hipMalloc failed for the outputs");
    auto run = [&]() -> gh_status {
        if (d_bc.p) GH_HIP(hipMemsetAsync(d_bc.p, 0, 8 * n, h->stream));
        if (d_ld.p) GH_HIP(hipMemsetAsync(d_ld.p, 0, 8 * n, h->stream));
        if (d_cnt.p) GH_HIP(hipMemsetAsync(d_cnt.p, 0, 16 * groups * 64, h->stream));
        for (int64_t g0 = 0; g0 < groups; g0 += G) {
            const int64_t gb = std::min(G, groups - g0);
            const int64_t ns = std::min<int64_t>(64 * gb, n_sources - 64 * g0);
            GH_TRY_ST(cent_run_batch(h, gb, sources + 64 * g0, ns, d_bc.p, d_ld.p, d_cnt.p ? d_cnt.p + 64 * g0 : nullptr,
                                     d_cnt.p ? d_cnt.p + 64 * groups + 64 * g0 : nullptr));
        }
        if (d_bc.p) GH_HIP(hipMemcpyAsync(betweenness, d_bc.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        if (d_ld.p) GH_HIP(hipMemcpyAsync(load, d_ld.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        if (d_cnt.p) {
            GH_HIP(hipMemcpyAsync(reached, d_cnt.p, 8 * n_sources, hipMemcpyDeviceToHost, h->stream));
            GH_HIP(hipMemcpyAsync(dist_sum, d_cnt.p + 64 * groups, 8 * n_sources, hipMemcpyDeviceToHost, h->stream));
        }
        GH_HIP(hipStreamSynchronize(h->stream));
        return GH_OK;
    };
    const gh_status st = run();
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);   // nothing is in flight when the outputs are freed
    return st;
}

extern "C" gh_status gh_cent_pagerank(gh_cent_handle h, double alpha, int32_t max_iter, double tol, double *x, int32_t *iterations) {
    if (!h) { g_cent_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(GH_ERR_INVALID, "alpha must be in [0, 1]");
    if (max_iter < 1) return fail(GH_ERR_INVALID, "max_iter must be >= 1");
    if (!(tol >= 0.0)) return fail(GH_ERR_INVALID, "tol must be >= 0");
    if (!x || !iterations) return fail(GH_ERR_INVALID, "x and iterations must not be NULL");
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    const int64_t n = h->n;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(PR_MAX_BLOCKS, (n + PR_BLOCK / 8 - 1) / (PR_BLOCK / 8)));
    gh_dev<double> d_x, d_part;
    gh_dev<PrState> d_st;
    if (!d_x.alloc(16 * n) || !d_part.alloc(16 * (size_t)nb) || !d_st.alloc(sizeof(PrState))) return fail(GH_ERR_NOMEM, "hipMalloc failed");
    double *xb[2] = {d_x.p, d_x.p + n};
    double *epart = d_part.p, *dpart = d_part.p + nb;
    auto run = [&]() -> gh_status {
        PrState hs{0.0, 0, 0};
        GH_HIP(hipMemcpyAsync(d_st.p, &hs, sizeof(hs), hipMemcpyHostToDevice, h->stream));
        pr_init_kernel<<<dim3(nb), dim3(PR_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, xb[0], dpart);
        pr_check_kernel<<<dim3(1), dim3(PR_BLOCK), 0, h->stream>>>(nb, epart, dpart, (double)n * tol, 0, max_iter, d_st.p);
        for (int32_t it = 1; it <= max_iter && !hs.done; ++it) {
            pr_step_kernel<<<dim3(nb), dim3(PR_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, h->d_adj.p, h->d_inv_deg.p, alpha, d_st.p,
                                                                        xb[(it - 1) & 1], xb[it & 1], epart, dpart);
            pr_check_kernel<<<dim3(1), dim3(PR_BLOCK), 0, h->stream>>>(nb, epart, dpart, (double)n * tol, it, max_iter, d_st.p);
            GH_HIP(hipGetLastError());
            if (it % PR_CHECK_EVERY == 0 || it == max_iter) {
                GH_HIP(hipMemcpyAsync(&hs, d_st.p, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
                GH_HIP(hipStreamSynchronize(h->stream));
            }
        }
        const int32_t last = hs.iters > 0 ? hs.iters : max_iter;
        GH_HIP(hipMemcpyAsync(x, xb[last & 1], 8 * n, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        *iterations = hs.iters;
        return GH_OK;
    };
    const gh_status st = run();
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);   // nothing is in flight when the buffers are freed
    return st;
}

extern "C" gh_status gh_spmv_adj_shift(void *hip_stream, int64_t n, const int64_t *indptr, const int32_t *indices, double c,
                                       const double *x, double *y) {
    if (n < 0 || (n > 0 && (!indptr || !indices || !x || !y))) { g_cent_error = "bad SpMV arguments"; return GH_ERR_INVALID; }
    if (n == 0) return GH_OK;
    const int64_t threads = 8 * n;
    spmv_adj_shift_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream>>>(n, indptr, indices, c, x, y);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_cent_error = std::string("spmv_adj_shift_kernel: ") + hipGetErrorString(e); return GH_ERR_HIP; }
    return GH_OK;
}
