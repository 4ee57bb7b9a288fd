// Run-time value -> compile-time template argument, for every kernel that is instantiated per embedding
// dimension D or per row stride LD.  The table D -> LD and the set of dimensions with kernels of their own are
// stated here and nowhere else.  No HIP header: a host compiler alone builds this file
// (tools/dispatch_host_check.cpp).
//
// A launch site holds its launch in one generic lambda:
//   if (!gh_dispatch_dim(h->D, [&](auto d, auto ld) { kernel<d(), ld()><<<grid, block, 0, stream>>>(args); }))
//       /* the generic kernel, or an error naming the site */;
#pragma once
#include <type_traits>

#if defined(__HIPCC__)
#define GH_HOST_DEVICE __host__ __device__
#else
#define GH_HOST_DEVICE
#endif

template <int V>
using gh_int = std::integral_constant<int, V>;

// Row stride (floats) of the padded position array for an embedding dimension D:
// rows are 16-byte aligned so a vertex is fetched with dwordx4 loads.
GH_HOST_DEVICE constexpr int gh_ld(int D) {
    return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : ((D + 3) & ~3);
}

// Embedding dimensions with compile-time kernels (spring pull, fused spring+scan, hub sums, intersection
// pairs) -- the domain of gh_dispatch_dim: every D from 2 to 16, so that e.g. n_components = 6 does not fall
// onto the generic one-thread-per-vertex kernels (2.4-2.8x slower at 1M vertices); larger D use those.  The
// norm order (gh_sumsq<D>) is the reference's for every D, so each D is its own instantiation rather than a
// padded neighbour.
GH_HOST_DEVICE constexpr bool gh_dim_templated(int D) {
    return D >= 2 && D <= 16;
}

// f(gh_int<Vi>{}) for the Vi equal to v -> true; no match: f is not called -> false.
template <int... Vs, class F>
bool gh_dispatch_value(int v, F &&f) {
    return ((v == Vs && (f(gh_int<Vs>{}), true)) || ...);
}

// f(gh_int<D>{}, gh_int<gh_ld(D)>{}) for a templated dimension -> true; any other D -> false.
template <class F>
bool gh_dispatch_dim(int D, F &&f) {
    static_assert(gh_dim_templated(2) && gh_dim_templated(16) && !gh_dim_templated(1) && !gh_dim_templated(17), "the list below");
    return gh_dispatch_value<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(D, [&](auto d) { f(d, gh_int<gh_ld(d())>{}); });
}

// f(gh_int<LD>{}) for the row strides of the templated dimensions -> true; any other stride -> false.
template <class F>
bool gh_dispatch_stride(int LD, F &&f) {
    return gh_dispatch_value<4, 8, 16>(LD, f);
}
