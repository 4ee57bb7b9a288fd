// The CSR builder (graphem-rapids_amd/csrc/csr_build.h) as a stand-alone host program:
//
//     g++ -std=c++17 -Wall -Werror tools/csr_build_host_check.cpp -o csr_build_host_check && ./csr_build_host_check
//     (the same with -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all for a run under the sanitizers)
//
// The rule, restated here without the builder's key order: row u is the sorted set of u's distinct neighbours other than u
// itself -- both endpoints' rows take the other one (symmetric), the first one's row takes the second (by source), or the
// second one's row takes the first (by target).  Every input below goes through gh_canonical_edge_keys and
// gh_csr_from_keys in all three shapes and is compared with that.  Exit status 0: every check held
// (tests/test_csr_build_host.py).
#include <cstdio>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../graphem-rapids_amd/csrc/csr_build.h"

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++failures; } } while (0)

static void check_graph(const char *name, int64_t n, const std::vector<int32_t> &pairs) {
    const int64_t count = (int64_t)pairs.size() / 2;
    for (gh_csr_shape shape : {GH_CSR_SYMMETRIC, GH_CSR_BY_SOURCE, GH_CSR_BY_TARGET}) {
        std::vector<std::set<int32_t>> rows((size_t)n);
        for (int64_t i = 0; i < count; ++i) {
            const int32_t u = pairs[2 * i], v = pairs[2 * i + 1];
            if (u == v) continue;
            if (shape != GH_CSR_BY_TARGET) rows[u].insert(v);
            if (shape != GH_CSR_BY_SOURCE) rows[v].insert(u);
        }
        std::vector<int64_t> want_ptr(1, 0);
        std::vector<int32_t> want_adj;
        for (const auto &row : rows) {
            want_adj.insert(want_adj.end(), row.begin(), row.end());   // a set iterates in ascending order
            want_ptr.push_back((int64_t)want_adj.size());
        }
        std::vector<uint64_t> keys;
        std::string err;
        std::vector<int64_t> ptr(3, -1);   // stale contents must not survive
        std::vector<int32_t> adj(5, -1);
        CHECK(gh_canonical_edge_keys(n, count, pairs.data(), shape != GH_CSR_SYMMETRIC, "edge", &keys, &err) == GH_OK);
        CHECK(err.empty());
        gh_csr_from_keys(n, keys, shape, &ptr, &adj);
        if (ptr != want_ptr || adj != want_adj) {
            std::fprintf(stderr, "%s, shape %d: the CSR differs from the rule\n", name, (int)shape);
            ++failures;
        }
        CHECK((int64_t)keys.size() * (shape == GH_CSR_SYMMETRIC ? 2 : 1) == (int64_t)adj.size());
    }
}

int main() {
    check_graph("one vertex", 1, {});
    check_graph("one edge, twice and reversed", 2, {0, 1, 1, 0, 0, 1});
    check_graph("self-loops only", 3, {0, 0, 2, 2, 1, 1, 2, 2});
    {
        std::vector<int32_t> star;   // hub 5 of 71 vertices, its 70 neighbours in descending order
        for (int32_t v = 70; v >= 0; --v)
            if (v != 5) { star.push_back(5); star.push_back(v); }
        CHECK(star.size() == 140);
        check_graph("star, descending", 71, star);
    }
    {
        std::mt19937 rng(20240607u);
        std::vector<int32_t> pairs;
        for (int i = 0; i < 360; ++i) pairs.push_back((int32_t)(rng() % 40));
        for (int i = 0; i < 20; ++i) pairs.insert(pairs.end(), {pairs[4 * i + (i & 1)], pairs[4 * i + 1 - (i & 1)]});   // repeats for certain, every other one reversed
        CHECK(pairs.size() == 400);
        check_graph("random pairs with repeats", 40, pairs);
    }

    // an id outside [0, n): GH_ERR_INVALID, and the message names the pair
    for (int32_t bad : {-1, 4}) {
        for (int side = 0; side < 2; ++side) {
            std::vector<int32_t> pairs = {0, 1, 2, 3, 1, 2};
            pairs[2 * 2 + side] = bad;
            std::vector<uint64_t> keys;
            std::string err;
            CHECK(gh_canonical_edge_keys(4, 3, pairs.data(), side == 1, "arc", &keys, &err) == GH_ERR_INVALID);
            CHECK(err == "arc 2 has a vertex id outside [0, n)");
        }
    }

    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("csr_build_host_check: ok\n");
    return 0;
}
