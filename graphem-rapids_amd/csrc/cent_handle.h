// The centrality handle (include/graphem_hip.h "centrality"), shared by centrality.hip, which owns its life cycle, and
// graphstats.hip, which reads the CSR, the stream and the budget and reports through err.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#define CENT_DEFAULT_BUDGET (1ll << 30)

struct gh_cent {
    int device = 0;
    int64_t n = 0, edges = 0;
    hipStream_t stream = nullptr;
    int64_t *d_ptr = nullptr;
    int32_t *d_adj = nullptr;
    double *d_inv_deg = nullptr;
    int64_t budget = CENT_DEFAULT_BUDGET;
    // path state for G groups, grown on demand
    int64_t cap_groups = 0;
    int32_t *d_dist = nullptr, *d_npred = nullptr, *d_flags = nullptr, *d_src = nullptr;
    double *d_sigma = nullptr, *d_delta = nullptr, *d_lam = nullptr;
    uint64_t *d_vis = nullptr, *d_fa = nullptr, *d_fb = nullptr;
    int2 *d_range = nullptr;
    std::string err;
};
