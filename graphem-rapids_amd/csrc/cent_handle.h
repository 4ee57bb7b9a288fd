// The centrality handle (include/graphem_hip.h "centrality"), shared by centrality.hip, which owns its life cycle, and
// graphstats.hip, communities.hip, cores.hip and links.hip, which read the CSR, the stream and the budget and report
// through err.  The CSR is gh_csr_from_keys' (csr_build.h): symmetric, deduplicated, rows ascending.
#pragma once
#include "host_util.h"

#define CENT_DEFAULT_BUDGET (1ll << 30)

// One level graph of communities.hip: CSR with weights, self weights and weighted degrees (level 0 reads the handle's CSR).
struct cent_level_graph {
    gh_dev<int64_t> ptr, self, k;
    gh_dev<int32_t> adj;
    gh_dev<uint32_t> wgt;
    void reset() { ptr.reset(); self.reset(); k.reset(); adj.reset(); wgt.reset(); }
};

struct gh_cent : gh_host {
    int64_t n = 0, edges = 0, max_degree = 0;
    gh_dev<int64_t> d_ptr;
    gh_dev<int32_t> d_adj;
    gh_dev<double> d_inv_deg;
    // path state for G groups, grown on demand
    int64_t cap_groups = 0;
    gh_dev<int32_t> d_dist, d_npred, d_flags, d_src;
    gh_dev<double> d_sigma, d_delta, d_lam;
    gh_dev<uint64_t> d_vis, d_fa, d_fb;
    gh_dev<int2> d_range;
    // the current and the next level graph of a gh_cent_louvain call; released when the call returns
    cent_level_graph lv[2];
    // links.hip: W_aa over 0 .. max_degree, built by the first link call and kept
    gh_dev<int64_t> d_link_aa;
};

// (centrality.hip) the message gh_cent_last_error(NULL) returns on this thread
void cent_set_create_error(const std::string &msg);
