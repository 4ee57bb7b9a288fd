// The collection of reverse-reachable sets behind gh_rr_* (include/graphem_hip.h "reverse influence sampling"): a CSR of
// sets on the device.  influence.hip appends sampled sets to it, ris.hip owns its life cycle, maximum coverage and counting.
#pragma once
#include "host_util.h"

#define RR_DEFAULT_BUDGET (4ll << 30)

struct gh_rr : gh_host {
    int64_t n = 0;
    int64_t sets = 0, members = 0;           // in use
    int64_t cap_sets = 0, cap_members = 0;   // allocated
    gh_dev<int64_t> d_indptr;                // (cap_sets + 1); d_indptr[0] = 0 always
    gh_dev<int32_t> d_members, d_roots;      // members ascending within a set; root -1 for an uploaded set
};

// bytes the budget counts for a collection of this size
inline int64_t rr_bytes(int64_t sets, int64_t members) { return 8 * (sets + 1) + 4 * sets + 4 * members; }

// Room for `sets` sets with `members` members in all; what is in use is kept.  Work is queued on `stream`.  A size past the
// budget is GH_ERR_NOMEM (the caller words the message), a failed hipMalloc too.
inline gh_status rr_reserve(gh_rr *h, int64_t sets, int64_t members, hipStream_t stream) {
    if (rr_bytes(sets, members) > h->budget) return GH_ERR_NOMEM;
    if (sets > h->cap_sets || !h->d_indptr.p) {
        const int64_t cap = std::max<int64_t>({sets, 2 * h->cap_sets, 64});
        gh_dev<int64_t> ip;
        gh_dev<int32_t> rt;
        if (!ip.alloc(8 * (cap + 1)) || !rt.alloc(4 * cap)) { h->err = "hipMalloc failed for the collection's offsets"; return GH_ERR_NOMEM; }
        if (h->d_indptr.p) {
            GH_HIP(hipMemcpyAsync(ip.p, h->d_indptr.p, 8 * (h->sets + 1), hipMemcpyDeviceToDevice, stream));
            GH_HIP(hipMemcpyAsync(rt.p, h->d_roots.p, 4 * h->sets, hipMemcpyDeviceToDevice, stream));
        } else {
            GH_HIP(hipMemsetAsync(ip.p, 0, 8, stream));
        }
        GH_HIP(hipStreamSynchronize(stream));   // the old buffers go now
        h->d_indptr = std::move(ip);
        h->d_roots = std::move(rt);
        h->cap_sets = cap;
    }
    if (members > h->cap_members) {
        // doubling, but never past what the budget leaves for members
        const int64_t most = (h->budget - 8 * (sets + 1) - 4 * sets) / 4;
        const int64_t cap = std::max<int64_t>(members, std::min<int64_t>(2 * h->cap_members, most));
        gh_dev<int32_t> mb;
        if (!mb.alloc(4 * cap)) { h->err = "hipMalloc failed for " + std::to_string(cap) + " members"; return GH_ERR_NOMEM; }
        if (h->members > 0) GH_HIP(hipMemcpyAsync(mb.p, h->d_members.p, 4 * h->members, hipMemcpyDeviceToDevice, stream));
        GH_HIP(hipStreamSynchronize(stream));
        h->d_members = std::move(mb);
        h->cap_members = cap;
    }
    return GH_OK;
}
