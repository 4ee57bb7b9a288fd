// Collections of reverse-reachable sets (include/graphem_hip.h "reverse influence sampling"): life cycle, upload and
// download, greedy maximum coverage and hit counting on the device.  The sets themselves are drawn in influence.hip.
//
// Maximum coverage: the transpose (vertex -> sets) is built once per call by count, scan and scatter.  A round is two
// launches and no host wait: rr_argmax_kernel reduces the packed key (uncovered count << 32 | 0xFFFFFFFF - id) over the
// vertices not yet chosen -- a wave by shuffles, a block through LDS, one 8-byte atomicMax per block -- and
// rr_cover_kernel reads the winner from device memory, takes a wave per set of that vertex, marks a set that was still
// uncovered and decrements the count of each of its members with integer atomics.  Every set is covered once over the
// whole call, so the work is the members in all plus k * n.  The k keys come back in one copy.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "rr_handle.h"

#define RR_BLOCK 256
#define RR_MAX_BLOCKS 1024
#define RR_COVER_BLOCKS 256         // rr_cover_kernel: a wave per set of the chosen vertex

static thread_local std::string g_rr_error;

namespace {

inline int rr_blocks(int64_t threads) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(RR_MAX_BLOCKS, (threads + RR_BLOCK - 1) / RR_BLOCK));
}

__global__ __launch_bounds__(RR_BLOCK) void rr_vcount_kernel(const int32_t *__restrict__ members, int64_t total, int32_t *cnt) {
    for (int64_t i = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RR_BLOCK)
        atomicAdd(&cnt[members[i]], 1);
}

// a wave per set: vsets[vptr[v] + slot] = s for every member v of set s
__global__ __launch_bounds__(RR_BLOCK) void rr_vscatter_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ members,
                                                              int64_t sets, const int64_t *__restrict__ vptr, int32_t *cursor,
                                                              int32_t *vsets) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (RR_BLOCK / 64);
    for (int64_t s = (int64_t)blockIdx.x * (RR_BLOCK / 64) + (threadIdx.x >> 6); s < sets; s += nwaves) {
        const int64_t beg = indptr[s], end = indptr[s + 1];
        for (int64_t i = beg + lane; i < end; i += 64) {
            const int32_t v = members[i];
            vsets[vptr[v] + atomicAdd(&cursor[v], 1)] = (int32_t)s;
        }
    }
}

__global__ __launch_bounds__(RR_BLOCK) void rr_argmax_kernel(const int32_t *__restrict__ cnt, const uint8_t *__restrict__ chosen,
                                                            int64_t n, unsigned long long *best) {
    __shared__ unsigned long long part[RR_BLOCK / 64];
    unsigned long long key = 0;   // every vertex's key is >= 2^31, so 0 never wins against one
    for (int64_t v = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * RR_BLOCK)
        if (!chosen[v]) key = max(key, ((unsigned long long)(uint32_t)cnt[v] << 32) | (0xFFFFFFFFu - (uint32_t)v));
    for (int d = 32; d > 0; d >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RR_BLOCK / 64; ++w) key = max(key, part[w]);
        if (key) atomicMax(best, key);
    }
}

__global__ __launch_bounds__(RR_BLOCK) void rr_cover_kernel(const unsigned long long *__restrict__ best,
                                                           const int64_t *__restrict__ indptr, const int32_t *__restrict__ members,
                                                           const int64_t *__restrict__ vptr, const int32_t *__restrict__ vsets,
                                                           uint8_t *covered, uint8_t *chosen, int32_t *cnt) {
    const unsigned long long key = *best;
    if (key == 0) return;   // no vertex left (the host asks for at most n rounds)
    const int32_t v = (int32_t)(0xFFFFFFFFu - (uint32_t)key);
    if (blockIdx.x == 0 && threadIdx.x == 0) chosen[v] = 1;
    if ((key >> 32) == 0) return;   // nothing left to cover through v
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (RR_BLOCK / 64);
    const int64_t beg = vptr[v], end = vptr[v + 1];
    for (int64_t q = beg + (int64_t)blockIdx.x * (RR_BLOCK / 64) + (threadIdx.x >> 6); q < end; q += nwaves) {
        const int32_t s = vsets[q];   // each set is once in v's list, so one wave decides it
        if (covered[s]) continue;
        const int64_t mb = indptr[s], me = indptr[s + 1];
        for (int64_t i = mb + lane; i < me; i += 64) atomicSub(&cnt[members[i]], 1);
        if (lane == 0) covered[s] = 1;
    }
}

__global__ __launch_bounds__(RR_BLOCK) void rr_flag_kernel(const int32_t *__restrict__ verts, int64_t m, uint8_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (i < m) flag[verts[i]] = 1;
}

__global__ __launch_bounds__(RR_BLOCK) void rr_hit_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ members,
                                                         int64_t sets, const uint8_t *__restrict__ flag, unsigned long long *count) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (RR_BLOCK / 64);
    unsigned long long mine = 0;
    for (int64_t s = (int64_t)blockIdx.x * (RR_BLOCK / 64) + (threadIdx.x >> 6); s < sets; s += nwaves) {
        const int64_t beg = indptr[s], end = indptr[s + 1];
        bool hit = false;
        for (int64_t i0 = beg; i0 < end && !hit; i0 += 64) hit = __ballot(i0 + lane < end && flag[members[i0 + lane]]) != 0;
        mine += hit ? 1 : 0;
    }
    if (lane == 0 && mine) atomicAdd(count, mine);
}

struct RrWiden {
    __host__ __device__ int64_t operator()(int32_t x) const { return x; }
};

}  // namespace

extern "C" gh_status gh_rr_create(gh_rr_handle *out, int device_id, int64_t n) {
    auto fail = [&](gh_status st, const std::string &msg) { g_rr_error = msg; return st; };
    if (!out) return fail(GH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "n must be in [1, 2^31)");
    gh_rr *h = new gh_rr();
    h->budget = RR_DEFAULT_BUDGET;
    h->n = n;
    gh_status st = gh_host_open(h, device_id, &g_rr_error);
    if (st == GH_OK) {
        st = rr_reserve(h, 0, 0, h->stream);
        if (st != GH_OK) g_rr_error = h->err;
    }
    if (st != GH_OK) { gh_rr_destroy(h); return st; }
    *out = h;
    return GH_OK;
}

extern "C" void gh_rr_destroy(gh_rr_handle h) {
    if (!h) return;
    gh_host_close(h);
    delete h;
}

extern "C" const char *gh_rr_last_error(gh_rr_handle h) { return h ? h->err.c_str() : g_rr_error.c_str(); }

extern "C" gh_status gh_rr_set_memory_budget(gh_rr_handle h, int64_t bytes) {
    return gh_host_set_budget(h, bytes, RR_DEFAULT_BUDGET, &g_rr_error);
}

extern "C" gh_status gh_rr_counts(gh_rr_handle h, int64_t *n_sets, int64_t *n_members) {
    if (!h) { g_rr_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (n_sets) *n_sets = h->sets;
    if (n_members) *n_members = h->members;
    return GH_OK;
}

extern "C" gh_status gh_rr_download(gh_rr_handle h, int64_t *indptr, int32_t *members, int32_t *roots) {
    if (!h) { g_rr_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    if (indptr) GH_HIP(hipMemcpyAsync(indptr, h->d_indptr.p, 8 * (h->sets + 1), hipMemcpyDeviceToHost, h->stream));
    if (members && h->members > 0) GH_HIP(hipMemcpyAsync(members, h->d_members.p, 4 * h->members, hipMemcpyDeviceToHost, h->stream));
    if (roots && h->sets > 0) GH_HIP(hipMemcpyAsync(roots, h->d_roots.p, 4 * h->sets, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_rr_upload(gh_rr_handle h, int64_t n_sets, const int64_t *indptr, const int32_t *members, const int32_t *roots) {
    if (!h) { g_rr_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (n_sets < 0 || n_sets > INT32_MAX || !indptr) return fail(GH_ERR_INVALID, "bad set offsets");
    if (indptr[0] != 0) return fail(GH_ERR_INVALID, "indptr[0] must be 0");
    for (int64_t s = 0; s < n_sets; ++s)
        if (indptr[s + 1] < indptr[s]) return fail(GH_ERR_INVALID, "indptr must not decrease");
    const int64_t total = indptr[n_sets];
    if (total > 0 && !members) return fail(GH_ERR_INVALID, "members is NULL");
    for (int64_t s = 0; s < n_sets; ++s)
        for (int64_t i = indptr[s]; i < indptr[s + 1]; ++i) {
            if (members[i] < 0 || members[i] >= h->n) return fail(GH_ERR_INVALID, "member vertex id outside [0, n)");
            if (i > indptr[s] && members[i] <= members[i - 1])
                return fail(GH_ERR_INVALID, "the members of set " + std::to_string(s) + " must ascend strictly");
        }
    if (roots)
        for (int64_t s = 0; s < n_sets; ++s)
            if (roots[s] < -1 || roots[s] >= h->n) return fail(GH_ERR_INVALID, "root vertex id outside [0, n) (-1: none)");
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    const int64_t sets0 = h->sets, members0 = h->members;
    h->sets = h->members = 0;   // nothing to keep while the buffers grow
    const gh_status st = rr_reserve(h, n_sets, total, h->stream);
    if (st != GH_OK) {
        h->sets = sets0;
        h->members = members0;
        if (st == GH_ERR_NOMEM && h->err.empty()) h->err = "the collection would outgrow its memory budget";
        return st;
    }
    GH_HIP(hipMemcpyAsync(h->d_indptr.p, indptr, 8 * (n_sets + 1), hipMemcpyHostToDevice, h->stream));
    if (total > 0) GH_HIP(hipMemcpyAsync(h->d_members.p, members, 4 * total, hipMemcpyHostToDevice, h->stream));
    if (n_sets > 0) {
        if (roots) GH_HIP(hipMemcpyAsync(h->d_roots.p, roots, 4 * n_sets, hipMemcpyHostToDevice, h->stream));
        else GH_HIP(hipMemsetAsync(h->d_roots.p, 0xFF, 4 * n_sets, h->stream));
    }
    GH_HIP(hipStreamSynchronize(h->stream));
    h->sets = n_sets;
    h->members = total;
    return GH_OK;
}

extern "C" gh_status gh_rr_cover(gh_rr_handle h, int64_t k, int32_t *seeds, int64_t *gains) {
    if (!h) { g_rr_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (k < 0) return fail(GH_ERR_INVALID, "k must be >= 0");
    const int64_t rounds = std::min<int64_t>(k, h->n);
    if (rounds == 0) return GH_OK;
    if (h->n + 1 > INT32_MAX) return fail(GH_ERR_INVALID, "maximum coverage needs n < 2^31 - 1");
    if (!seeds || !gains) return fail(GH_ERR_INVALID, "seeds or gains is NULL");
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    const int64_t n = h->n, sets = h->sets, total = h->members;
    gh_dev<int32_t> d_cnt, d_cursor, d_vsets;
    gh_dev<int64_t> d_vptr;
    gh_dev<uint8_t> d_covered, d_chosen;
    gh_dev<unsigned long long> d_best;
    gh_dev<char> d_tmp;
    if (!d_cnt.alloc(4 * (n + 1)) || !d_cursor.alloc(4 * n) || !d_vsets.alloc(4 * total) || !d_vptr.alloc(8 * (n + 1)) ||
        !d_covered.alloc(sets) || !d_chosen.alloc(n) || !d_best.alloc(8 * rounds))
        return fail(GH_ERR_NOMEM, "hipMalloc failed for the vertex-to-sets transpose");
    GH_HIP(hipMemsetAsync(d_cnt.p, 0, 4 * (n + 1), h->stream));
    GH_HIP(hipMemsetAsync(d_cursor.p, 0, 4 * n, h->stream));
    GH_HIP(hipMemsetAsync(d_covered.p, 0, std::max<int64_t>(sets, 1), h->stream));
    GH_HIP(hipMemsetAsync(d_chosen.p, 0, n, h->stream));
    GH_HIP(hipMemsetAsync(d_best.p, 0, 8 * rounds, h->stream));
    if (total > 0) {
        rr_vcount_kernel<<<dim3(rr_blocks(total)), dim3(RR_BLOCK), 0, h->stream>>>(h->d_members.p, total, d_cnt.p);
        GH_LAUNCH_CHECK();
    }
    hipcub::TransformInputIterator<int64_t, RrWiden, const int32_t *> wide(d_cnt.p, RrWiden());
    size_t temp = 0;
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, wide, d_vptr.p, (int)(n + 1), h->stream));
    if (!d_tmp.alloc(temp)) return fail(GH_ERR_NOMEM, "hipMalloc failed for scan scratch");
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, temp, wide, d_vptr.p, (int)(n + 1), h->stream));
    if (total > 0) {
        rr_vscatter_kernel<<<dim3(rr_blocks(sets * 64)), dim3(RR_BLOCK), 0, h->stream>>>(h->d_indptr.p, h->d_members.p, sets, d_vptr.p,
                                                                                        d_cursor.p, d_vsets.p);
        GH_LAUNCH_CHECK();
    }
    const int grid_n = rr_blocks(n), grid_c = RR_COVER_BLOCKS;
    for (int64_t r = 0; r < rounds; ++r) {
        rr_argmax_kernel<<<dim3(grid_n), dim3(RR_BLOCK), 0, h->stream>>>(d_cnt.p, d_chosen.p, n, d_best.p + r);
        rr_cover_kernel<<<dim3(grid_c), dim3(RR_BLOCK), 0, h->stream>>>(d_best.p + r, h->d_indptr.p, h->d_members.p, d_vptr.p, d_vsets.p,
                                                                       d_covered.p, d_chosen.p, d_cnt.p);
    }
    GH_LAUNCH_CHECK();
    std::vector<unsigned long long> best((size_t)rounds);
    GH_HIP(hipMemcpyAsync(best.data(), d_best.p, 8 * rounds, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    for (int64_t r = 0; r < rounds; ++r) {
        seeds[r] = (int32_t)(0xFFFFFFFFu - (uint32_t)best[r]);
        gains[r] = (int64_t)(best[r] >> 32);
    }
    return GH_OK;
}

extern "C" gh_status gh_rr_count_hit(gh_rr_handle h, const int32_t *vertices, int64_t m, int64_t *count) {
    if (!h) { g_rr_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (!count) return fail(GH_ERR_INVALID, "count is NULL");
    if (m < 0 || (m > 0 && !vertices)) return fail(GH_ERR_INVALID, "bad vertex set");
    for (int64_t i = 0; i < m; ++i)
        if (vertices[i] < 0 || vertices[i] >= h->n) return fail(GH_ERR_INVALID, "vertex id outside [0, n)");
    *count = 0;
    if (m == 0 || h->sets == 0) return GH_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    gh_dev<uint8_t> d_flag;
    gh_dev<int32_t> d_verts;
    gh_dev<unsigned long long> d_count;
    if (!d_flag.alloc(h->n) || !d_verts.alloc(4 * m) || !d_count.alloc(8)) return fail(GH_ERR_NOMEM, "hipMalloc failed for the vertex flags");
    GH_HIP(hipMemsetAsync(d_flag.p, 0, h->n, h->stream));
    GH_HIP(hipMemsetAsync(d_count.p, 0, 8, h->stream));
    GH_HIP(hipMemcpyAsync(d_verts.p, vertices, 4 * m, hipMemcpyHostToDevice, h->stream));
    rr_flag_kernel<<<dim3((unsigned)((m + RR_BLOCK - 1) / RR_BLOCK)), dim3(RR_BLOCK), 0, h->stream>>>(d_verts.p, m, d_flag.p);
    rr_hit_kernel<<<dim3(rr_blocks(h->sets * 64)), dim3(RR_BLOCK), 0, h->stream>>>(h->d_indptr.p, h->d_members.p, h->sets, d_flag.p,
                                                                                  d_count.p);
    GH_LAUNCH_CHECK();
    unsigned long long c = 0;
    GH_HIP(hipMemcpyAsync(&c, d_count.p, 8, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    *count = (int64_t)c;
    return GH_OK;
}
