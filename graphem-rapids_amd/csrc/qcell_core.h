#pragma once
// Cell table of the query balls: the pre-filter of phase B in the fused kernel for D <= 3 (fused.hip,
// spring_scan_cells_kernel).  Instead of screening every (query, midpoint) pair of a tile, it indexes the S query
// balls -- a table of a few KB, built once per launch -- and a midpoint runs the exact test against the queries whose
// ball can reach its cell only.
//
// Cell frame.  Per axis G - 1 boundaries b_0 <= .. <= b_{G-2}, taken at equal-count quantiles of a sample of the
// query coordinates.  A coordinate's cell is the number of boundaries <= it (gh_qc_axis_cell): monotone, and the end
// cells run to -inf / +inf, so outliers far from the core cost nothing.  The boundaries only decide how well the table
// filters, never which pairs pass: any set of values (NaN included -- it is never <= anything) gives the same
// candidates.
//
// Box of a query (gh_qc_axis_box): the cells of one axis that a midpoint m with exact fp32 d2(q, m) <= tau can lie in.
// Why it is conservative, for the chain of `park` (d2 = fma(df_{D-1}, df_{D-1}, ... fma(df_0, df_0, 0)), df = q - m
// rounded to fp32):
//   (1) d2 >= fma(df_d, df_d, 0) for every axis d: each fma adds a non-negative term and rounding is monotone.
//   (2) For a boundary b <= q and any m < b: q - m > q - b >= 0, so fl(q - m) >= fl(q - b) and
//       fma(fl(q - m), .., 0) >= fma(fl(q - b), .., 0) (rounding is monotone).  If the latter is > tau, no m below b
//       passes, and b is counted in every passing m's cell: lo = #{b <= q : fma(fl(q - b)^2) > tau}.
//   (3) Mirror image for b > q and m >= b (fl(q - m) = -fl(m - q): round-to-nearest is symmetric):
//       only the boundaries above q that are NOT that far can be <= a passing m, so
//       hi = #{b <= q} + #{b > q : fma(fl(q - b)^2) <= tau}.
// So the test is the kernel's own fp32 arithmetic applied to the boundaries: no square root, no margin, no rounding
// mode to get right.  Flushing denormals to zero is monotone too, so (2) and (3) hold in either mode.
// tests/test_query_cells_cpu.py checks it on the host copy of this code (gh_qcell_probe).
//
// Table (one blob of GH_QC_WORDS u32, the layout below): CSR from cell to query indices (uint8: S <= 256) plus a wide
// list.  A query is wide when its tau or a coordinate is not finite, when its box has more than GH_QC_CAP cells, or when
// its cells would take the entries past GH_QC_ENT (boxes counted in query order); every midpoint tests every wide query.
// So the CSR cannot overflow.  The cap trades the scan against the build: on the rr1m bench state (tau taken as the
// 700th distance, offline) a cap of 8 cells sends 7 queries to the wide list and a wave makes ~27 tests per pair of
// midpoints, 14 of them wide; a cap of 27, 2 and ~17; a cap of 64, none and ~13 -- but there the builder's loops over
// a box (two per query, one of returning atomics) published the table so late that a tenth of the workgroups waited
// ~10 us for it (tools/stamp_probe.py).
#include "common.h"
#include "engine.h"   // GH_CT_M; GH_QC_SMAX, GH_CT_KMAX (step_plan.h)

#define GH_QC_G 8                                 // cells per axis
#define GH_QC_CAP 27                              // cells a query's box may cover before it goes on the wide list
#define GH_QC_ENT 2048                            // entries of the CSR
// (GH_QC_SMAX, the queries -- one staged group, one uint8 index: step_plan.h)
#define GH_QC_CELLS (GH_QC_G * GH_QC_G * GH_QC_G)  // D = 3 (D = 2 uses the first G * G)
#define GH_QC_SAMPLE 64                           // queries whose coordinates place the boundaries (one wave)
// blob layout, in u32 words
#define GH_QC_OFF_NWIDE 0                         // [0] wide count
#define GH_QC_OFF_B 4                             // 3 axes x 8 floats: G - 1 boundaries, then one unused
#define GH_QC_OFF_PTR 28                          // GH_QC_CELLS + 1 uint16 offsets into the entries
#define GH_QC_OFF_ENT 288                         // GH_QC_ENT uint8 query indices, by cell
#define GH_QC_OFF_WIDE (GH_QC_OFF_ENT + GH_QC_ENT / 4)                 // GH_QC_SMAX uint8 query indices
#define GH_QC_TAB_WORDS (GH_QC_OFF_WIDE + GH_QC_SMAX / 4)              // 864 words = 216 x 16 bytes: the table proper
// behind the table in the device buffer (not in a workgroup's LDS copy of it): the S query records (x, y, z|0, tau) that
// workgroup 0 publishes with it when it computes the thresholds itself (gh_ct_tau)
#define GH_QC_OFF_REC GH_QC_TAB_WORDS
#define GH_QC_WORDS (GH_QC_OFF_REC + 4 * GH_QC_SMAX)
static_assert(GH_QC_OFF_B + 3 * 8 <= GH_QC_OFF_PTR, "blob layout");
static_assert(GH_QC_OFF_PTR + (GH_QC_CELLS + 2) / 2 <= GH_QC_OFF_ENT, "blob layout");
static_assert(GH_QC_TAB_WORDS % 4 == 0 && GH_QC_WORDS % 4 == 0, "the blob moves in 16-byte pieces");

__host__ __device__ inline int gh_qc_axis_cell(const float *b, float x) {
    int c = 0;
#pragma unroll
    for (int i = 0; i < GH_QC_G - 1; ++i) c += b[i] <= x ? 1 : 0;
    return c;
}

__host__ __device__ inline void gh_qc_axis_box(const float *b, float q, float tau, int &lo, int &hi) {
    lo = 0;
    hi = 0;
#pragma unroll
    for (int i = 0; i < GH_QC_G - 1; ++i) {
        const float df = q - b[i];
        const bool far = fmaf(df, df, 0.0f) > tau;   // the first step of park's chain, on the boundary
        if (b[i] <= q) { lo += far ? 1 : 0; hi += 1; }
        else hi += far ? 0 : 1;
    }
}

// Exclusive prefix sum of one value per thread over a workgroup of NT threads (in thread order), and the total.
template <int NT>
__device__ __forceinline__ uint32_t gh_qc_block_scan(uint32_t v, uint32_t *wsum /* NT / 64 */, uint32_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = __shfl_up(incl, o, 64);
        if (lane >= o) incl += x;
    }
    __syncthreads();   // wsum may still be read by a previous scan
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int ww = 0; ww < NT / 64; ++ww) {
        base += ww < w ? wsum[ww] : 0;
        total += wsum[ww];
    }
    return base + incl - v;
}

// tau of one query from its GH_CT_M coarse group minima (setup_core.h "COARSE FORM"), by ONE thread: the K-th smallest of
// them AS A MULTISET (copies count, see gh_tau_kth), K <= KC, kept as KC ascending registers that every value is passed
// through (a min and a max per register and value).  Fewer than K occupied groups: +inf -- the query goes on the wide list
// and, should its candidate list overflow, to the exact fallback.  The loads are independent of one another and plain (the
// launch in front wrote the table); the consumed entries are reset for the set-up after the next.
// The values pass in batches of B in a loop that is NOT unrolled, the loads of a batch issued while the batch before it is
// sorted in; B is the caller's: what its register budget allows (fused.hip).  Written without the loop, the compiler keeps
// every ADDRESS in registers too (160 - 250 VGPRs for the fused kernel: three or two workgroups per CU instead of five, for
// the sake of the launch's first one).
// Measured on rr1m (tools/stamp_probe.py, workgroup 0 of the fused launch, which shares its CU with four gathering
// workgroups): B = 16: 6.0 us, B = 64: 3.8 - 4.2 us.  Not faster, each tried on top of B = 64: the first batch fetched before
// the cell frame and sorted in behind it (5.3 us behind a 3 us frame), one v_med3_u32 per register and value instead of
// min + max, reading the lower neighbour's old value so that no step waits for another (5.2 - 6.3 us), the same in a loop
// over slices of 8 registers, for its code size (5.9 - 7.8 us), s_setprio 3 (4.9 us with the median form).
template <int KC, int B /* values per batch */>
__device__ __forceinline__ float gh_ct_tau(uint32_t *cmin, uint32_t q /* the query */, uint32_t S, int K) {
    static_assert(GH_CT_M % B == 0, "whole batches");
    uint32_t a[KC], cur[B], nxt[B];
#pragma unroll
    for (int i = 0; i < KC; ++i) a[i] = 0x7F800000u;
#pragma unroll
    for (int j = 0; j < B; ++j) cur[j] = cmin[q + (uint32_t)j * S];
#pragma unroll 1
    for (uint32_t b = 0; b < GH_CT_M / B; ++b) {
        uint32_t *row = cmin + q + b * B * S;   // (entry j of this batch; the next batch starts B rows on)
        if (b + 1 < GH_CT_M / B) {
#pragma unroll
            for (int j = 0; j < B; ++j) nxt[j] = row[(uint32_t)(B + j) * S];
        }
#pragma unroll
        for (int j = 0; j < B; ++j) row[(uint32_t)j * S] = GH_CT_EMPTY;
#pragma unroll
        for (int j = 0; j < B; ++j) {
            uint32_t x = cur[j];   // (an empty entry, 0xFFFFFFFF, or the bits of a NaN: sinks through, every register stays <= +inf)
#pragma unroll
            for (int i = 0; i < KC; ++i) {
                const uint32_t lo = min(a[i], x);
                x = max(a[i], x);
                a[i] = lo;
            }
        }
#pragma unroll
        for (int j = 0; j < B; ++j) cur[j] = nxt[j];
    }
    uint32_t kth = 0x7F800000u;   // K > KC cannot be (the launcher checks): +inf all the same
#pragma unroll
    for (int i = 0; i < KC; ++i) kth = i == K - 1 ? a[i] : kth;
    return __uint_as_float(kth);
}

// Built by ONE workgroup of NT >= 256 threads (the first of the fused launch) from the query records (x, y, z|0, tau) --
// thread t < S hands in record t -- S <= GH_QC_SMAX, in the LDS blob `tab`; scratch: 4 KB of records, GH_QC_CELLS
// counters.  Ends with the blob complete in `tab` and the records in `rec` (after a barrier).
// Two halves: gh_qc_frame -- records to LDS, the cell frame -- needs the coordinates only; gh_qc_fill, which takes the
// thresholds (r.w), does the rest.
template <int D, int NT>
__device__ __forceinline__ void gh_qc_frame(float4 r, int S, uint32_t *tab, float4 *rec, uint32_t *cnt,
                                            unsigned long long *st = nullptr /* diagnostic: thread 0's stamps of the stages */) {
    static_assert(NT >= GH_QC_SMAX, "one query per thread");
    constexpr int NC = D == 3 ? GH_QC_CELLS : GH_QC_G * GH_QC_G;
    const int t = threadIdx.x;
    if (t < S) rec[t] = r;
    for (int c = t; c < NC; c += NT) cnt[c] = 0;
    if (t == 0) tab[GH_QC_OFF_NWIDE] = 0;
    __syncthreads();
    if (st) st[0] = wall_clock64();
    // boundaries: wave d < D ranks an evenly spaced sample of the coordinates of axis d (ties by lane), lane of rank
    // floor(i * n / G) supplies boundary i - 1
    float *bnd = reinterpret_cast<float *>(tab + GH_QC_OFF_B);
    const int w = t >> 6, lane = t & 63;
    if (w < D) {
        const int n = min(S, GH_QC_SAMPLE);
        const float4 sr = lane < n ? rec[(int)(((int64_t)lane * S) / n)] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float x = w == 0 ? sr.x : w == 1 ? sr.y : sr.z;
        const uint32_t u = __float_as_uint(x);
        const uint32_t key = lane < n ? ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) : 0xFFFFFFFFu;   // total order
        // (all GH_QC_SAMPLE lanes, unrolled: the lanes past n hold the largest key and are never counted by a lane below n;
        // a loop over the first n with the lane in a register took 3.8 us of this workgroup's critical path)
        int rank = 0;
#pragma unroll
        for (int p = 0; p < GH_QC_SAMPLE; ++p) {
            const uint32_t kp = (uint32_t)__builtin_amdgcn_readlane((int)key, p);
            rank += (kp < key || (kp == key && p < lane)) ? 1 : 0;
        }
        if (lane < n) {
#pragma unroll
            for (int i = 1; i < GH_QC_G; ++i)
                if (rank == (i * n) / GH_QC_G) bnd[w * 8 + i - 1] = x;
        }
    }
    __syncthreads();
    if (st) st[1] = wall_clock64();
}
template <int D, int NT>
__device__ __forceinline__ void gh_qc_fill(float4 r, int S, uint32_t *tab, float4 *rec, uint32_t *cnt, unsigned long long *st = nullptr) {
    constexpr int NC = D == 3 ? GH_QC_CELLS : GH_QC_G * GH_QC_G;
    const int t = threadIdx.x;
    if (t < S) rec[t].w = r.w;   // (own slot; nobody reads a threshold from LDS before the barriers below)
    else r = make_float4(0.f, 0.f, 0.f, -1.f);
    const float *bnd = reinterpret_cast<const float *>(tab + GH_QC_OFF_B);
    // boxes: counted per cell, or the query goes on the wide list
    __shared__ uint32_t wsum[NT / 64];
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool listed = false;
    int ncell = 0;
    uint8_t *wide = reinterpret_cast<uint8_t *>(tab + GH_QC_OFF_WIDE);
    if (t < S) {
        const float q[3] = {r.x, r.y, r.z};
        bool finite = isfinite(r.w);
        ncell = 1;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            finite = finite && isfinite(q[d]);
            gh_qc_axis_box(bnd + d * 8, q[d], r.w, lo[d], hi[d]);
            ncell *= hi[d] - lo[d] + 1;
        }
        listed = finite && ncell <= GH_QC_CAP;
    }
    {   // the entries of the listed boxes, in query order, up to GH_QC_ENT
        uint32_t total;
        const uint32_t before = gh_qc_block_scan<NT>(listed ? (uint32_t)ncell : 0u, wsum, total);
        listed = listed && before + (uint32_t)ncell <= GH_QC_ENT;
    }
    if (t < S && !listed) wide[atomicAdd(&tab[GH_QC_OFF_NWIDE], 1u)] = (uint8_t)t;
    if (st) st[2] = wall_clock64();
    // The cells of a box, x fastest, by three counters.  (The k-th cell by division -- k % wx, (k / wx) % wy, k / (wx wy),
    // four integer divisions per cell and loop -- made the build 10.4 us of this workgroup's 11.5: unnoticed while the
    // thresholds came from a launch of their own and the table was ready before the first workgroups asked for it.)
    const int wx = hi[0] - lo[0] + 1, wy = hi[1] - lo[1] + 1;
    struct box_walk {
        int x = 0, y = 0, z = 0;
        __device__ __forceinline__ int next(const int (&lo)[3], int wx, int wy) {   // the current cell; moves on
            const int c = (lo[0] + x) + GH_QC_G * ((lo[1] + y) + GH_QC_G * (lo[2] + z));
            if (++x == wx) { x = 0; if (++y == wy) { y = 0; ++z; } }
            return c;
        }
    };
    if (listed) {
        box_walk wk;
        for (int k = 0; k < ncell; ++k) atomicAdd(&cnt[wk.next(lo, wx, wy)], 1u);   // (no return value: nothing to wait for)
    }
    __syncthreads();
    if (st) st[3] = wall_clock64();
    // offsets: exclusive sum of the counters (thread t owns cells 2t, 2t + 1; NC <= 2 NT), then cnt = fill cursors
    uint16_t *ptr = reinterpret_cast<uint16_t *>(tab + GH_QC_OFF_PTR);
    {
        static_assert(GH_QC_CELLS <= 2 * NT, "two cells per thread");
        const uint32_t a = 2 * t < NC ? cnt[2 * t] : 0, b = 2 * t + 1 < NC ? cnt[2 * t + 1] : 0;
        uint32_t total;
        const uint32_t ex = gh_qc_block_scan<NT>(a + b, wsum, total);
        if (2 * t < NC) { ptr[2 * t] = (uint16_t)ex; cnt[2 * t] = ex; }
        if (2 * t + 1 < NC) { ptr[2 * t + 1] = (uint16_t)(ex + a); cnt[2 * t + 1] = ex + a; }
        if (t == 0) ptr[NC] = (uint16_t)total;
    }
    __syncthreads();
    if (st) st[4] = wall_clock64();
    uint8_t *ent = reinterpret_cast<uint8_t *>(tab + GH_QC_OFF_ENT);
    // four returning atomics in flight at a time (the loops over a box are what made the table late at a cap of 64)
    if (listed) {
        box_walk wk;
        for (int k0 = 0; k0 < ncell; k0 += 4) {
            uint32_t at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = wk.next(lo, wx, wy);   // (past the box's last cell: not used)
                at[u] = k0 + u < ncell ? atomicAdd(&cnt[c], 1u) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + u < ncell) ent[at[u]] = (uint8_t)t;
        }
    }
    __syncthreads();
}
template <int D, int NT>
__device__ __forceinline__ void gh_qc_build(float4 r, int S, uint32_t *tab, float4 *rec, uint32_t *cnt, unsigned long long *st = nullptr) {
    gh_qc_frame<D, NT>(r, S, tab, rec, cnt, st);
    gh_qc_fill<D, NT>(r, S, tab, rec, cnt, st);
}
