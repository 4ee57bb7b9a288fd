// The dimension / stride dispatchers (graphem-rapids_amd/csrc/dispatch.h) as a stand-alone host program:
//
//     g++ -std=c++17 tools/dispatch_host_check.cpp -o dispatch_host_check && ./dispatch_host_check
//     (the same with -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all for a run under the sanitizers)
//
// Checks, for every run-time value in and around the domains, that the callback runs exactly once with the matching
// compile-time constants and not at all outside the domain, that the return value says which, and that gh_ld is the table
// the kernels were written for.  Exit status 0: every check held (tests/test_dispatch_host.py).
#include <cstdio>
#include <vector>

#include "../graphem-rapids_amd/csrc/dispatch.h"

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++failures; } } while (0)

struct call { int a, b; };

int main() {
    // gh_ld: the expression common.h held before the table moved
    for (int D = 1; D <= 64; ++D) CHECK(gh_ld(D) == (D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : ((D + 3) & ~3)));
    static_assert(gh_ld(3) == 4 && gh_ld(5) == 8 && gh_ld(16) == 16 && gh_ld(17) == 20, "usable as a template argument");

    for (int D = 0; D <= 40; ++D) {
        std::vector<call> calls;
        const bool hit = gh_dispatch_dim(D, [&](auto d, auto ld) {
            static_assert(decltype(ld)::value == gh_ld(decltype(d)::value), "the stride constant belongs to the dimension constant");
            calls.push_back(call{d(), ld()});
        });
        const bool in = D >= 2 && D <= 16;
        CHECK(hit == in);
        CHECK(hit == gh_dim_templated(D));
        CHECK(calls.size() == (in ? 1u : 0u));
        if (in && calls.size() == 1) CHECK(calls[0].a == D && calls[0].b == gh_ld(D));
    }

    for (int LD = 0; LD <= 40; ++LD) {
        std::vector<call> calls;
        const bool hit = gh_dispatch_stride(LD, [&](auto ld) { calls.push_back(call{ld(), 0}); });
        const bool in = LD == 4 || LD == 8 || LD == 16;
        CHECK(hit == in);
        CHECK(calls.size() == (in ? 1u : 0u));
        if (in && calls.size() == 1) CHECK(calls[0].a == LD);
    }

    // an arbitrary list (the float64 engine's): unordered, 0 as a member, the match in the last place; and the empty list
    for (int v = -3; v <= 40; ++v) {
        std::vector<call> calls;
        const bool hit = gh_dispatch_value<2, 3, 4, 5, 6, 8, 16, 0>(v, [&](auto c) { calls.push_back(call{c(), 0}); });
        const bool in = v == 0 || (v >= 2 && v <= 6) || v == 8 || v == 16;
        CHECK(hit == in);
        CHECK(calls.size() == (in ? 1u : 0u));
        if (in && calls.size() == 1) CHECK(calls[0].a == v);
        int none = 0;
        CHECK(!gh_dispatch_value<>(v, [&](auto) { ++none; }));
        CHECK(none == 0);
        int one = 0;
        CHECK(gh_dispatch_value<7>(v, [&](auto c) { one += c(); }) == (v == 7));
        CHECK(one == (v == 7 ? 7 : 0));
    }
    // a value listed twice runs once: the first match ends the search
    int twice = 0;
    CHECK(gh_dispatch_value<5, 5>(5, [&](auto) { ++twice; }) && twice == 1);

    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("dispatch_host_check: ok\n");
    return 0;
}
