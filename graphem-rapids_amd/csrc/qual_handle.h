// The layout-quality handle (include/graphem_hip.h "layout quality"), shared by quality.hip, which owns its life cycle and
// the position snapshot, and clusters.hip and classify.hip, which read the snapshot, the stream and the device and report
// through err.  With it: the float32 distance chain all of them evaluate, and the host thread pool of their host paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "host_util.h"

#define QUAL_BLOCK 256
#define QUAL_HOST_THREADS 16

// The exact-difference chain of the header: (((0 + t_0 t_0) + t_1 t_1) + ...), t_d = a[d] - b[d * sb], every operation a
// separate float32 operation (the Makefile's -ffp-contract=off keeps the product and the sum apart).  a is a packed row; b
// has stride sb, which is 1 for a packed row and the tile's column count for a column of the staged tile.
__host__ __device__ __forceinline__ float qual_d2(const float *a, const float *b, int64_t sb, int D) {
    float s = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float t = a[d] - b[d * sb];
        s = s + t * t;
    }
    return s;
}

// The same chain between two packed rows of a dimension known to the compiler: a row held in registers stays there.
template <int DT> __host__ __device__ __forceinline__ float qual_d2_fixed(const float *a, const float *b) {
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        const float t = a[d] - b[d];
        s = s + t * t;
    }
    return s;
}

struct gh_qual : gh_host {          // device < 0: host path
    int64_t n = 0, E = 0;
    int32_t D = 0;                  // 0: no positions yet
    int64_t epoch = 0;              // counts the snapshots taken: what clusters.hip keeps per snapshot names its epoch
    size_t pos_bytes = 0;
    gh_dev<int2> d_edges;
    gh_dev<float> d_pos;            // the snapshot, packed (n, D)
    gh_dev<float4> d_seg;
    std::vector<int2> h_edges;
    std::vector<float> h_pos;
    std::vector<float4> h_seg;
    // the simple graph of the edge list (self-loops dropped, repeats and both directions merged), built by the first
    // neighbour query: neighbours of u = g_idx[g_ptr[u] .. g_ptr[u + 1]), ids ascending
    bool g_built = false;
    std::vector<int64_t> g_ptr;
    std::vector<int32_t> g_idx;
    gh_dev<int64_t> d_gptr;         // the same on the device, uploaded by the first hop profile
    gh_dev<int32_t> d_gidx;
    // clusters.hip: the scan of the snapshot (greatest |x| as float32 bits, first row with a NaN or an infinity, -1: none)
    // and the running minimum of gh_qual_kmeans_seed_step, each with the epoch it belongs to
    int64_t scan_epoch = -1, bad_row = -1, seed_epoch = -1;
    uint32_t max_abs_bits = 0;
    gh_dev<float> d_min_d2;
    std::vector<float> h_min_d2;
};

// (quality.hip) the message gh_qual_last_error(NULL) returns on this thread
void qual_set_create_error(const std::string &msg);

// (clusters.hip) the scan of the snapshot, once per epoch: GH_ERR_INVALID "position row <v> is not finite" for a row with a NaN
// or an infinity
gh_status cl_scan(gh_qual *h);

inline gh_status qual_invalid(gh_qual *h, const std::string &msg) {
    h->err = msg;
    return GH_ERR_INVALID;
}

// fn(first, last) over [0, count) on up to QUAL_HOST_THREADS threads
template <class Fn> void qual_host_parallel(int64_t count, int64_t grain, Fn fn) {
    const int64_t want = std::min<int64_t>(QUAL_HOST_THREADS, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    const int64_t nt = std::max<int64_t>(1, std::min(want, count / std::max<int64_t>(1, grain)));
    if (nt == 1) { fn(0, count); return; }
    std::vector<std::thread> pool;
    for (int64_t t = 0; t < nt; ++t) pool.emplace_back(fn, count * t / nt, count * (t + 1) / nt);
    for (auto &th : pool) th.join();
}

inline unsigned qual_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + QUAL_BLOCK - 1) / QUAL_BLOCK); }
