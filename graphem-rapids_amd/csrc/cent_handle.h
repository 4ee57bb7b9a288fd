// The centrality handle (include/graphem_hip.h "centrality"), shared by centrality.hip, which owns its life cycle, and
// graphstats.hip, which reads the CSR, the stream and the budget and reports through err.
#pragma once
#include "host_util.h"

#define CENT_DEFAULT_BUDGET (1ll << 30)

struct gh_cent : gh_host {
    int64_t n = 0, edges = 0;
    gh_dev<int64_t> d_ptr;
    gh_dev<int32_t> d_adj;
    gh_dev<double> d_inv_deg;
    // path state for G groups, grown on demand
    int64_t cap_groups = 0;
    gh_dev<int32_t> d_dist, d_npred, d_flags, d_src;
    gh_dev<double> d_sigma, d_delta, d_lam;
    gh_dev<uint64_t> d_vis, d_fa, d_fb;
    gh_dev<int2> d_range;
};

// (centrality.hip) the message gh_cent_last_error(NULL) returns on this thread
void cent_set_create_error(const std::string &msg);
