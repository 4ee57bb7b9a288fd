// From vertex pairs to a CSR, for every handle that keeps a graph (centrality.hip, quality.hip, influence.hip): the canonical
// edge set as ascending keys, and the one builder from those keys to (ptr, adj).  The rule: row u holds the sorted set of
// u's distinct neighbours other than u itself.  No HIP header: a host compiler reads this file alone
// (tools/csr_build_host_check.cpp restates the rule and compares).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"

// The canonical edge set of `count` vertex pairs on n vertices: ids validated, self-loops dropped, duplicates merged, as
// ascending keys (a << 32) | b -- (u, v) as given when directed, else (min, max).  `noun` names a pair in the message.
inline gh_status gh_canonical_edge_keys(int64_t n, int64_t count, const int32_t *pairs, bool directed, const char *noun,
                                        std::vector<uint64_t> *keys, std::string *err) {
    keys->clear();
    keys->reserve((size_t)count);
    for (int64_t i = 0; i < count; ++i) {
        const int64_t u = pairs[2 * i], v = pairs[2 * i + 1];
        if (u < 0 || u >= n || v < 0 || v >= n) {
            *err = std::string(noun) + " " + std::to_string(i) + " has a vertex id outside [0, n)";
            return GH_ERR_INVALID;
        }
        if (u == v) continue;
        const uint64_t a = directed ? u : std::min(u, v), b = directed ? v : std::max(u, v);
        keys->push_back((a << 32) | b);
    }
    std::sort(keys->begin(), keys->end());
    keys->erase(std::unique(keys->begin(), keys->end()), keys->end());
    return GH_OK;
}

// Which rows a key (a, b) enters: both (undirected keys, a < b), row a only (the arcs by source), row b only (by target).
enum gh_csr_shape { GH_CSR_SYMMETRIC, GH_CSR_BY_SOURCE, GH_CSR_BY_TARGET };

// The CSR of ascending canonical keys: neighbours of u = adj[ptr[u] .. ptr[u + 1]), ascending without a sort.  The keys
// ascend by (a, b), so a row b is handed its a's in ascending order and a row a its b's; a symmetric row takes the a's
// first, which are all below it, and then the b's, which are all above.
inline void gh_csr_from_keys(int64_t n, const std::vector<uint64_t> &keys, gh_csr_shape shape, std::vector<int64_t> *ptr,
                             std::vector<int32_t> *adj) {
    const bool by_a = shape != GH_CSR_BY_TARGET, by_b = shape != GH_CSR_BY_SOURCE;
    ptr->assign((size_t)n + 1, 0);
    for (uint64_t k : keys) {
        if (by_a) ++(*ptr)[(size_t)(k >> 32) + 1];
        if (by_b) ++(*ptr)[(size_t)(k & 0xFFFFFFFFu) + 1];
    }
    for (int64_t u = 0; u < n; ++u) (*ptr)[u + 1] += (*ptr)[u];
    adj->resize((size_t)(*ptr)[n]);
    std::vector<int64_t> fill(ptr->begin(), ptr->end() - 1);
    if (by_b) for (uint64_t k : keys) (*adj)[(size_t)fill[k & 0xFFFFFFFFu]++] = (int32_t)(k >> 32);
    if (by_a) for (uint64_t k : keys) (*adj)[(size_t)fill[k >> 32]++] = (int32_t)(k & 0xFFFFFFFFu);
}
