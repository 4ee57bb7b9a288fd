// Spearman rank correlation, plain and over bootstrap resamples (include/graphem_hip.h "rank correlation";
// graphem-rapids_amd/visualization.py).
//
// A resample is a vector of multiplicities c over the original points, so no replicate sorts anything: a column is
// sorted once when the handle is made, and per replicate its midranks follow from a prefix sum of c along that order.
// Everything up to the three sums of a pair is integer arithmetic; gh_corr_rho turns them into a double on the host.
//
//   create     corr_key_kernel (order-preserving keys), hipCUB radix sort of (key, point), corr_groups_kernel (per
//              sorted position the first position of its tie group and the one after its last, by binary search).
//   counts     corr_counts_kernel: one lane per draw, one integer atomic add into the replicate's count table.  A count
//              is at most n < 2^21, so a 32-bit table cannot overflow.
//   ranks      corr_scan_kernel: one workgroup per (replicate, column) walks the column's order in tiles and writes the
//              exclusive prefix E of c along it (E[n] = n).  corr_rank_kernel: u = E[group start] + E[group end] - n per
//              sorted position, stored at the point's own index.
//   moments    corr_moments_kernel: per (replicate, pair) the sums of c u v, c u u, c v v in int64; a wave tree, an LDS
//              step over the waves, then one integer atomic per sum and workgroup.  Integer addition is associative,
//              so no order has to be kept.
// The host path (device_id < 0) runs the same rules in plain loops, replicates spread over a few threads.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "host_util.h"

#define CORR_GOLDEN 0x9E3779B97F4A7C15ull
#define CORR_BLOCK 256
#define CORR_SCAN_BLOCK 1024
#define CORR_SCAN_ITEMS 4
#define CORR_SCAN_TILE (CORR_SCAN_BLOCK * CORR_SCAN_ITEMS)
#define CORR_SCAN_WAVES (CORR_SCAN_BLOCK / 64)
#define CORR_MAX_BATCH 4096
#define CORR_MAX_X_BLOCKS 4096
#define CORR_DEFAULT_BUDGET (4ll << 30)
#define CORR_HOST_THREADS 16

namespace {

__host__ __device__ __forceinline__ uint64_t corr_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t corr_stream(uint64_t seed, uint64_t i) { return corr_mix(seed + (i + 1) * CORR_GOLDEN); }
__host__ __device__ __forceinline__ uint64_t corr_word(uint64_t stream, uint64_t j) { return corr_mix(stream ^ j); }

__host__ __device__ __forceinline__ uint64_t corr_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Ascending doubles -> ascending keys; -0.0 and 0.0 share a key.
__host__ __device__ __forceinline__ uint64_t corr_key(double x) {
    if (x == 0.0) x = 0.0;
    union { double d; uint64_t u; } v;
    v.d = x;
    return (v.u >> 63) ? ~v.u : v.u | 0x8000000000000000ull;
}

inline int64_t corr_pad4(int64_t x) { return (x + 3) & ~(int64_t)3; }

__global__ __launch_bounds__(CORR_BLOCK) void corr_key_kernel(int64_t n, const double *__restrict__ col, uint64_t *keys, uint32_t *ids) {
    const int64_t i = (int64_t)blockIdx.x * CORR_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = corr_key(col[i]);
    ids[i] = (uint32_t)i;
}

// gs[k] = the first sorted position with key[k]'s value, ge[k] = the position after the last one
__global__ __launch_bounds__(CORR_BLOCK) void corr_groups_kernel(int64_t n, const uint64_t *__restrict__ skeys, int32_t *gs, int32_t *ge) {
    const int64_t k = (int64_t)blockIdx.x * CORR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = skeys[k];
    int64_t lo = 0, hi = k;                    // the first position whose key is >= key
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (skeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    gs[k] = (int32_t)lo;
    lo = k + 1; hi = n;                        // the first position whose key is > key
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (skeys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    ge[k] = (int32_t)lo;
}

// c[b * ns + idx(b0 + b, j)] += 1; blockIdx.y = replicate of the batch
__global__ __launch_bounds__(CORR_BLOCK) void corr_counts_kernel(int64_t n, int64_t ns, uint64_t seed, int64_t b0, uint32_t *c) {
    const uint64_t stream = corr_stream(seed, (uint64_t)(b0 + blockIdx.y));
    uint32_t *mine = c + (int64_t)blockIdx.y * ns;
    for (int64_t j = (int64_t)blockIdx.x * CORR_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * CORR_BLOCK) {
        const uint64_t idx = corr_mulhi(corr_word(stream, (uint64_t)j), (uint64_t)n);   // < n
        atomicAdd(mine + idx, 1u);
    }
}

// Workgroup (slot = blockIdx.x, replicate = blockIdx.y): E[k] = the sum of c[order[j]] over j < k, k = 0 .. n.
// order rows have stride ns, E rows stride es, both multiples of 4, so the 16-byte accesses are aligned.
__global__ __launch_bounds__(CORR_SCAN_BLOCK) void corr_scan_kernel(int64_t n, int64_t ns, int64_t es, const uint32_t *__restrict__ c,
                                                                   const int32_t *__restrict__ order, const int32_t *__restrict__ ucols,
                                                                   int32_t ncu, uint32_t *E) {
    __shared__ uint32_t wave_sum[2][CORR_SCAN_WAVES];
    const int32_t slot = blockIdx.x;
    const int64_t b = blockIdx.y;
    const uint32_t *cb = c + b * ns;
    const int32_t *ord = order + (int64_t)ucols[slot] * ns;
    uint32_t *Eb = E + (b * ncu + slot) * es;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    int buf = 0;
    // the values of the tile after this one are fetched while this one is scanned
    uint32_t nxt[CORR_SCAN_ITEMS];
    auto fetch = [&](int64_t k0) {
        if (k0 + CORR_SCAN_ITEMS <= n) {
            const int4 o = *reinterpret_cast<const int4 *>(ord + k0);
            nxt[0] = cb[o.x]; nxt[1] = cb[o.y]; nxt[2] = cb[o.z]; nxt[3] = cb[o.w];
        } else {
            for (int q = 0; q < CORR_SCAN_ITEMS; ++q) nxt[q] = k0 + q < n ? cb[ord[k0 + q]] : 0u;
        }
    };
    fetch((int64_t)threadIdx.x * CORR_SCAN_ITEMS);
    for (int64_t t0 = 0; t0 < n; t0 += CORR_SCAN_TILE) {
        const int64_t k0 = t0 + (int64_t)threadIdx.x * CORR_SCAN_ITEMS;
        uint32_t v[CORR_SCAN_ITEMS];
        for (int q = 0; q < CORR_SCAN_ITEMS; ++q) v[q] = nxt[q];
        if (t0 + CORR_SCAN_TILE < n) fetch(k0 + CORR_SCAN_TILE);
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        uint32_t incl = mine;                  // inclusive scan over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[buf][wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < CORR_SCAN_WAVES; ++w) {
            const uint32_t s = wave_sum[buf][w];
            if (w < wave) before += s;
            total += s;
        }
        buf ^= 1;                              // the next tile writes the other row: one barrier per tile
        uint32_t e = carry + before + incl - mine;
        if (k0 + CORR_SCAN_ITEMS <= n) {
            uint4 out;
            out.x = e; e += v[0];
            out.y = e; e += v[1];
            out.z = e; e += v[2];
            out.w = e;
            *reinterpret_cast<uint4 *>(Eb + k0) = out;
        } else {
            for (int q = 0; q < CORR_SCAN_ITEMS; ++q) {
                if (k0 + q < n) Eb[k0 + q] = e;
                e += v[q];
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) Eb[n] = carry;
}

// u[point at sorted position k] = E[gs[k]] + E[ge[k]] - n; blockIdx.y = slot, blockIdx.z = replicate
__global__ __launch_bounds__(CORR_BLOCK) void corr_rank_kernel(int64_t n, int64_t ns, int64_t es, const int32_t *__restrict__ order,
                                                              const int32_t *__restrict__ gs, const int32_t *__restrict__ ge,
                                                              const int32_t *__restrict__ ucols, int32_t ncu,
                                                              const uint32_t *__restrict__ E, int32_t *u) {
    const int64_t col = ucols[blockIdx.y];
    const int64_t seg = (int64_t)blockIdx.z * ncu + blockIdx.y;
    const uint32_t *Eb = E + seg * es;
    int32_t *ub = u + seg * ns;
    for (int64_t k = (int64_t)blockIdx.x * CORR_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * CORR_BLOCK) {
        const int64_t at = col * ns + k;
        ub[order[at]] = (int32_t)(Eb[gs[at]] + Eb[ge[at]]) - (int32_t)n;
    }
}

__device__ __forceinline__ int64_t corr_wave_sum(int64_t x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
    return x;
}

// sums[(replicate * n_pairs + pair) * 3 + {0, 1, 2}] += this workgroup's share; blockIdx.y = pair, blockIdx.z = replicate
__global__ __launch_bounds__(CORR_BLOCK) void corr_moments_kernel(int64_t n, int64_t ns, const uint32_t *__restrict__ c,
                                                                 const int32_t *__restrict__ u, const int32_t *__restrict__ pair_slots,
                                                                 int32_t ncu, int32_t n_pairs, unsigned long long *sums) {
    __shared__ int64_t part[CORR_BLOCK / 64][3];
    const int64_t b = blockIdx.z;
    const uint32_t *cb = c + b * ns;
    const int32_t *ux = u + (b * ncu + pair_slots[2 * blockIdx.y]) * ns;
    const int32_t *uy = u + (b * ncu + pair_slots[2 * blockIdx.y + 1]) * ns;
    int64_t sxy = 0, sxx = 0, syy = 0;
    for (int64_t i = (int64_t)blockIdx.x * CORR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CORR_BLOCK) {
        const int64_t w = cb[i], x = ux[i], y = uy[i];
        const int64_t wx = w * x;
        sxy += wx * y;
        sxx += wx * x;
        syy += w * y * y;
    }
    sxy = corr_wave_sum(sxy);
    sxx = corr_wave_sum(sxx);
    syy = corr_wave_sum(syy);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { part[wave][0] = sxy; part[wave][1] = sxx; part[wave][2] = syy; }
    __syncthreads();
    if (threadIdx.x < 3) {
        int64_t s = 0;
        for (int w = 0; w < CORR_BLOCK / 64; ++w) s += part[w][threadIdx.x];
        atomicAdd(sums + (b * n_pairs + blockIdx.y) * 3 + threadIdx.x, (unsigned long long)s);   // two's complement: wraps to the signed sum
    }
}

inline unsigned corr_grid(int64_t items) {
    return (unsigned)std::min<int64_t>(CORR_MAX_X_BLOCKS, std::max<int64_t>(1, (items + CORR_BLOCK - 1) / CORR_BLOCK));
}

}  // namespace

struct gh_corr : gh_host {          // device < 0: host path
    int64_t n = 0, ns = 0, es = 0;   // points; row strides of order / gs / ge / c / u and of E (multiples of 4)
    int32_t m = 0;
    // per column and sorted position: the point, its tie group's first position and the position after its last
    gh_dev<int32_t> d_order, d_gs, d_ge;
    std::vector<int32_t> h_order, h_gs, h_ge;
};

static thread_local std::string g_corr_error;

namespace {

gh_status corr_prepare_device(gh_corr *h, const double *columns) {
    const int64_t n = h->n, ns = h->ns;
    const size_t table = 4 * (size_t)ns * h->m;
    if (!h->d_order.alloc(table) || !h->d_gs.alloc(table) || !h->d_ge.alloc(table)) {
        h->err = "hipMalloc failed for " + std::to_string(3 * table) + " bytes of column order";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemsetAsync(h->d_order.p, 0, table, h->stream));   // the padding of every row is a valid point
    gh_dev<double> d_col;
    gh_dev<uint64_t> d_keys, d_skeys;
    gh_dev<uint32_t> d_ids;
    gh_dev<void> d_tmp;
    if (!d_col.alloc(8 * n) || !d_keys.alloc(8 * n) || !d_skeys.alloc(8 * n) || !d_ids.alloc(4 * n)) {
        h->err = "hipMalloc failed for the sort buffers";
        return GH_ERR_NOMEM;
    }
    size_t temp = 0;
    GH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp, d_keys.p, d_skeys.p, d_ids.p,
                                                (uint32_t *)h->d_order.p, (int)n, 0, 64, h->stream));
    if (!d_tmp.alloc(temp)) { h->err = "hipMalloc failed for the sort's work space"; return GH_ERR_NOMEM; }
    const dim3 blk(CORR_BLOCK), grd((unsigned)((n + CORR_BLOCK - 1) / CORR_BLOCK));
    for (int32_t col = 0; col < h->m; ++col) {
        GH_HIP(hipMemcpyAsync(d_col.p, columns + (int64_t)col * n, 8 * n, hipMemcpyHostToDevice, h->stream));
        corr_key_kernel<<<grd, blk, 0, h->stream>>>(n, d_col.p, d_keys.p, d_ids.p);
        GH_HIP(hipGetLastError());
        GH_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, temp, d_keys.p, d_skeys.p, d_ids.p,
                                                    (uint32_t *)(h->d_order.p + (int64_t)col * ns), (int)n, 0, 64, h->stream));
        corr_groups_kernel<<<grd, blk, 0, h->stream>>>(n, d_skeys.p, h->d_gs.p + (int64_t)col * ns, h->d_ge.p + (int64_t)col * ns);
        GH_HIP(hipGetLastError());
    }
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

void corr_prepare_host(gh_corr *h, const double *columns) {
    const int64_t n = h->n;
    h->h_order.resize((size_t)n * h->m);
    h->h_gs.resize((size_t)n * h->m);
    h->h_ge.resize((size_t)n * h->m);
    std::vector<std::pair<uint64_t, int32_t>> keyed((size_t)n);
    for (int32_t col = 0; col < h->m; ++col) {
        for (int64_t i = 0; i < n; ++i) keyed[i] = {corr_key(columns[(int64_t)col * n + i]), (int32_t)i};
        std::sort(keyed.begin(), keyed.end());
        int32_t *order = h->h_order.data() + (int64_t)col * n, *gs = h->h_gs.data() + (int64_t)col * n, *ge = h->h_ge.data() + (int64_t)col * n;
        for (int64_t k = 0; k < n; ++k) {
            order[k] = keyed[k].second;
            gs[k] = k > 0 && keyed[k].first == keyed[k - 1].first ? gs[k - 1] : (int32_t)k;
        }
        for (int64_t k = n - 1; k >= 0; --k) ge[k] = k + 1 < n && keyed[k].first == keyed[k + 1].first ? ge[k + 1] : (int32_t)(k + 1);
    }
}

// The columns that occur in the pairs, ascending, and every pair as two positions in that list.
void corr_slots(int32_t m, int32_t n_pairs, const int32_t *pairs, std::vector<int32_t> &ucols, std::vector<int32_t> &pair_slots) {
    std::vector<int32_t> slot_of((size_t)m, -1);
    for (int32_t p = 0; p < 2 * n_pairs; ++p) slot_of[pairs[p]] = 0;
    ucols.clear();
    for (int32_t col = 0; col < m; ++col)
        if (slot_of[col] == 0) { slot_of[col] = (int32_t)ucols.size(); ucols.push_back(col); }
    pair_slots.resize(2 * (size_t)n_pairs);
    for (int32_t p = 0; p < 2 * n_pairs; ++p) pair_slots[p] = slot_of[pairs[p]];
}

// Host path: the sums of replicates b = first, first + step, .. (plain statistic: reps = 1 and c = 1).
void corr_host_range(const gh_corr *h, bool plain, int32_t first, int32_t step, int32_t reps, uint64_t seed,
                     const std::vector<int32_t> &ucols, const std::vector<int32_t> &pair_slots, int64_t *sums) {
    const int64_t n = h->n;
    const int32_t ncu = (int32_t)ucols.size(), n_pairs = (int32_t)(pair_slots.size() / 2);
    std::vector<uint32_t> c((size_t)n), E((size_t)n + 1);
    std::vector<int32_t> u((size_t)n * ncu);
    for (int32_t b = first; b < reps; b += step) {
        if (plain) std::fill(c.begin(), c.end(), 1u);
        else {
            std::fill(c.begin(), c.end(), 0u);
            const uint64_t stream = corr_stream(seed, (uint64_t)b);
            for (int64_t j = 0; j < n; ++j) ++c[corr_mulhi(corr_word(stream, (uint64_t)j), (uint64_t)n)];
        }
        for (int32_t s = 0; s < ncu; ++s) {
            const int64_t base = (int64_t)ucols[s] * n;
            const int32_t *order = h->h_order.data() + base, *gs = h->h_gs.data() + base, *ge = h->h_ge.data() + base;
            uint32_t run = 0;
            for (int64_t k = 0; k < n; ++k) { E[k] = run; run += c[order[k]]; }
            E[n] = run;
            int32_t *us = u.data() + (int64_t)s * n;
            for (int64_t k = 0; k < n; ++k) us[order[k]] = (int32_t)(E[gs[k]] + E[ge[k]]) - (int32_t)n;
        }
        for (int32_t p = 0; p < n_pairs; ++p) {
            const int32_t *ux = u.data() + (int64_t)pair_slots[2 * p] * n, *uy = u.data() + (int64_t)pair_slots[2 * p + 1] * n;
            int64_t sxy = 0, sxx = 0, syy = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t w = c[i], x = ux[i], y = uy[i];
                sxy += w * x * y;
                sxx += w * x * x;
                syy += w * y * y;
            }
            int64_t *out = sums + ((int64_t)b * n_pairs + p) * 3;
            out[0] = sxy; out[1] = sxx; out[2] = syy;
        }
    }
}

void corr_host(const gh_corr *h, bool plain, int32_t reps, uint64_t seed, const std::vector<int32_t> &ucols,
               const std::vector<int32_t> &pair_slots, int64_t *sums) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int32_t workers = (int32_t)std::min<int64_t>({(int64_t)CORR_HOST_THREADS, (int64_t)hw, (int64_t)reps});
    if (workers <= 1) { corr_host_range(h, plain, 0, 1, reps, seed, ucols, pair_slots, sums); return; }
    std::vector<std::thread> pool;
    for (int32_t t = 0; t < workers; ++t)
        pool.emplace_back([=, &ucols, &pair_slots] { corr_host_range(h, plain, t, workers, reps, seed, ucols, pair_slots, sums); });
    for (auto &t : pool) t.join();
}

// Device path: sums (reps, n_pairs, 3) host, replicate-major.
gh_status corr_device(gh_corr *h, bool plain, int32_t reps, uint64_t seed, const std::vector<int32_t> &ucols,
                      const std::vector<int32_t> &pair_slots, int64_t *sums) {
    (void)hipSetDevice(h->device);
    const int64_t n = h->n, ns = h->ns, es = h->es;
    const int32_t ncu = (int32_t)ucols.size(), n_pairs = (int32_t)(pair_slots.size() / 2);
    const int64_t per_rep = 4 * ns + (int64_t)ncu * 4 * (ns + es) + 24 * (int64_t)n_pairs;
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>({(int64_t)reps, (int64_t)CORR_MAX_BATCH, h->budget / per_rep}));
    gh_dev<uint32_t> d_c, d_E;
    gh_dev<int32_t> d_u, d_ucols, d_slots;
    gh_dev<unsigned long long> d_sums;
    if (!d_c.alloc(4 * (size_t)(batch * ns)) || !d_E.alloc(4 * (size_t)(batch * ncu * es)) || !d_u.alloc(4 * (size_t)(batch * ncu * ns)) ||
        !d_ucols.alloc(4 * (size_t)ncu) || !d_slots.alloc(8 * (size_t)n_pairs) || !d_sums.alloc(24 * (size_t)(batch * n_pairs))) {
        h->err = "hipMalloc failed for " + std::to_string(batch) + " replicates of " + std::to_string(per_rep) + " bytes";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_ucols.p, ucols.data(), 4 * (size_t)ncu, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_slots.p, pair_slots.data(), 8 * (size_t)n_pairs, hipMemcpyHostToDevice, h->stream));
    const unsigned gx = corr_grid(n);
    const unsigned mx = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (n + 16 * CORR_BLOCK - 1) / (16 * CORR_BLOCK)));
    for (int64_t b0 = 0; b0 < reps; b0 += batch) {
        const int64_t nb = std::min<int64_t>(batch, reps - b0);
        if (plain) GH_HIP(hipMemsetD32Async((hipDeviceptr_t)d_c.p, 1, (size_t)(nb * ns), h->stream));
        else {
            GH_HIP(hipMemsetAsync(d_c.p, 0, 4 * (size_t)(nb * ns), h->stream));
            corr_counts_kernel<<<dim3(gx, (unsigned)nb), dim3(CORR_BLOCK), 0, h->stream>>>(n, ns, seed, b0, d_c.p);
            GH_HIP(hipGetLastError());
        }
        corr_scan_kernel<<<dim3((unsigned)ncu, (unsigned)nb), dim3(CORR_SCAN_BLOCK), 0, h->stream>>>(
            n, ns, es, d_c.p, h->d_order.p, d_ucols.p, ncu, d_E.p);
        GH_HIP(hipGetLastError());
        corr_rank_kernel<<<dim3(gx, (unsigned)ncu, (unsigned)nb), dim3(CORR_BLOCK), 0, h->stream>>>(
            n, ns, es, h->d_order.p, h->d_gs.p, h->d_ge.p, d_ucols.p, ncu, d_E.p, d_u.p);
        GH_HIP(hipGetLastError());
        GH_HIP(hipMemsetAsync(d_sums.p, 0, 24 * (size_t)(nb * n_pairs), h->stream));
        corr_moments_kernel<<<dim3(mx, (unsigned)n_pairs, (unsigned)nb), dim3(CORR_BLOCK), 0, h->stream>>>(
            n, ns, d_c.p, d_u.p, d_slots.p, ncu, n_pairs, d_sums.p);
        GH_HIP(hipGetLastError());
        GH_HIP(hipMemcpyAsync(sums + b0 * n_pairs * 3, d_sums.p, 24 * (size_t)(nb * n_pairs), hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
    }
    return GH_OK;
}

// sums (reps, n_pairs, 3), replicate-major, for the plain statistic (reps = 1) or the resamples
gh_status corr_run(gh_corr *h, bool plain, int32_t n_pairs, const int32_t *pairs, int32_t reps, uint64_t seed, std::vector<int64_t> &sums) {
    std::vector<int32_t> ucols, pair_slots;
    corr_slots(h->m, n_pairs, pairs, ucols, pair_slots);
    sums.assign((size_t)reps * n_pairs * 3, 0);
    if (h->device < 0) { corr_host(h, plain, reps, seed, ucols, pair_slots, sums.data()); return GH_OK; }
    return corr_device(h, plain, reps, seed, ucols, pair_slots, sums.data());
}

}  // namespace

extern "C" double gh_corr_rho(int64_t sxy, int64_t sxx, int64_t syy) {
    if (sxx == 0 || syy == 0) return std::numeric_limits<double>::quiet_NaN();
    return (double)sxy / std::sqrt((double)sxx * (double)syy);
}

extern "C" gh_status gh_corr_create(gh_corr_handle *out, int device_id, int64_t n, int32_t m, const double *columns) {
    if (!out) { g_corr_error = "out is NULL"; return GH_ERR_INVALID; }
    *out = nullptr;
    if (m < 1 || !columns) { g_corr_error = "at least one column is needed"; return GH_ERR_INVALID; }
    if (n < 2) { g_corr_error = "n must be at least 2, got " + std::to_string(n); return GH_ERR_INVALID; }
    if (n > GH_CORR_MAX_N) {
        g_corr_error = "n = " + std::to_string(n) + " is above " + std::to_string(GH_CORR_MAX_N) + ": the sums of n^3 terms would need 128-bit integers";
        return GH_ERR_INVALID;
    }
    for (int64_t i = 0; i < n * m; ++i)
        if (!std::isfinite(columns[i])) {
            g_corr_error = "column " + std::to_string(i / n) + " has a non-finite value at index " + std::to_string(i % n);
            return GH_ERR_INVALID;
        }
    gh_corr *h = new gh_corr();
    h->budget = CORR_DEFAULT_BUDGET;
    h->n = n;
    h->m = m;
    h->ns = corr_pad4(n);
    h->es = corr_pad4(n + 1);
    gh_status st = GH_OK;
    if (device_id < 0) corr_prepare_host(h, columns);
    else {
        st = gh_host_open(h, device_id, &g_corr_error);
        if (st == GH_OK && (st = corr_prepare_device(h, columns)) != GH_OK) g_corr_error = h->err;
    }
    if (st != GH_OK) { gh_corr_destroy(h); return st; }
    *out = h;
    return GH_OK;
}

extern "C" void gh_corr_destroy(gh_corr_handle h) {
    if (!h) return;
    gh_host_close(h);
    delete h;
}

extern "C" const char *gh_corr_last_error(gh_corr_handle h) { return h ? h->err.c_str() : g_corr_error.c_str(); }

extern "C" gh_status gh_corr_set_memory_budget(gh_corr_handle h, int64_t bytes) {
    return gh_host_set_budget(h, bytes, CORR_DEFAULT_BUDGET, &g_corr_error);
}

extern "C" gh_status gh_corr_matrix(gh_corr_handle h, double *out, int64_t *sums) {
    if (!h) { g_corr_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (!out) { h->err = "out is NULL"; return GH_ERR_INVALID; }
    const int32_t m = h->m;
    if ((int64_t)m * (m + 1) / 2 > 65535) { h->err = "the matrix of " + std::to_string(m) + " columns has more than 65535 entries"; return GH_ERR_INVALID; }
    std::vector<int32_t> pairs;                // every x <= y; the diagonal carries Sxx alone
    for (int32_t x = 0; x < m; ++x)
        for (int32_t y = x; y < m; ++y) { pairs.push_back(x); pairs.push_back(y); }
    std::vector<int64_t> s;
    const gh_status st = corr_run(h, true, (int32_t)(pairs.size() / 2), pairs.data(), 1, 0, s);
    if (st != GH_OK) return st;
    for (size_t p = 0; p < pairs.size() / 2; ++p) {
        const int32_t x = pairs[2 * p], y = pairs[2 * p + 1];
        const int64_t sxy = s[3 * p], sxx = s[3 * p + 1], syy = s[3 * p + 2];
        const double rho = x == y ? (sxx == 0 ? std::numeric_limits<double>::quiet_NaN() : 1.0) : gh_corr_rho(sxy, sxx, syy);
        out[(int64_t)x * m + y] = out[(int64_t)y * m + x] = rho;
        if (sums) {
            int64_t *a = sums + ((int64_t)x * m + y) * 3, *b = sums + ((int64_t)y * m + x) * 3;
            a[0] = sxy; a[1] = sxx; a[2] = syy;
            b[0] = sxy; b[1] = syy; b[2] = sxx;
        }
    }
    return GH_OK;
}

extern "C" gh_status gh_corr_bootstrap(gh_corr_handle h, int32_t n_pairs, const int32_t *pairs, int32_t reps, uint64_t seed,
                                       double *out, int64_t *sums) {
    if (!h) { g_corr_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](const std::string &msg) { h->err = msg; return GH_ERR_INVALID; };
    if (reps < 1) return fail("reps must be at least 1, got " + std::to_string(reps));
    if (n_pairs < 1 || !pairs) return fail("at least one pair is needed");
    if (n_pairs > 65535) return fail("more than 65535 pairs");
    if (!out) return fail("out is NULL");
    for (int32_t p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= h->m)
            return fail("pair " + std::to_string(p / 2) + " names column " + std::to_string(pairs[p]) + ", the table has " + std::to_string(h->m));
    std::vector<int64_t> s;
    const gh_status st = corr_run(h, false, n_pairs, pairs, reps, seed, s);
    if (st != GH_OK) return st;
    for (int64_t b = 0; b < reps; ++b)
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int64_t *t = s.data() + (b * n_pairs + p) * 3;
            out[p * reps + b] = gh_corr_rho(t[0], t[1], t[2]);
            if (sums) std::memcpy(sums + (p * reps + b) * 3, t, 24);
        }
    return GH_OK;
}
