// Fused spring + KNN scan: the dominant kernel of an iteration.
//
// Why fused: the spring pull is bound by the chip's rate for random row requests (8 neighbour rows
// of 16 bytes per vertex, ~65-73 G rows/s whatever the byte rate), the KNN scan by the matrix pipe /
// the fp32 VALU.  As separate kernels they run back to back (146 + 110 us on the 1M-vertex graph) and
// the midpoints make a round trip through memory.  Here one workgroup owns a range of consecutive own
// rows holding at most TILE owned edges (an edge is owned by ONE of its endpoints -- by a hash of the
// edge id, or by endpoint 0 for range partitions; bit 31 of a pull-list entry marks the edges a row owns):
//   phase A  spring pull of its vertices (reference pt.py:595-636, summation order of the
//            two index_add_ calls) -> Fs; the midpoints (pt.py:785) of the owned edges fall
//            out of the gathered rows and are kept in LDS, never written to memory;
//   phase B  those midpoints become the workgroup's reference tile: R per thread in packed
//            registers, all S queries stream past (scan_core.h).  For D <= 3 on graphs whose thresholds
//            have a launch of their own the queries are indexed instead: a cell table of their balls,
//            built by the launch's first workgroup, sends each midpoint to the few queries that can
//            reach it (qcell_core.h, spring_scan_cells_kernel).
// Workgroups in phase A (waiting on gathers) and workgroups in phase B (issuing VALU) share
// the CUs, so the two bounds overlap instead of adding.
#include "common.h"
#include "engine.h"
#include "qcell_core.h"
#include "scan_core.h"
#include "tau_core.h"

#include <stdio.h>
#include <stdlib.h>

// Fused-kernel geometry: 256 threads x 2 references per thread = tiles of 512 owned edges per workgroup.
// (Measured on the 1M-vertex graph, D = 3, before the matrix-pipe filter: 256x8 225 us, 256x4 197 us -- a smaller tile costs
// more filter work per pair but less LDS per workgroup, so more workgroups are resident and their gather / filter phases
// interleave better.)
// The pre-filter of phase B runs on the matrix pipe for every fused dimension: split-f16 operands for D <= 3 (1024 pairs per
// matrix instruction), single-piece f16 operands for 4 <= D <= 16 (scan_core.h).  Against the packed-fp32 VALU form it
// replaced (rounds 1-2; removed in round 4 together with its GRAPHEM_HIP_MFMA / _FUSED_CFG switches): 1M vertices, 256
// queries: 4700 vs 4440 it/s in the steady state of a long run; 100K vertices 10760 vs 9730; 1024 queries 433 vs 566 us per
// iteration, 4096 queries 640 vs 1434 us for the kernel; D = 12: 818 -> 508 us per iteration.
// (gh_plan_mfma, GH_FUSED_NT / _R / _TILE: step_plan.h)
//
// Workgroups of 256 threads, R = 2 references per thread: tiles of 512 owned edges (95 VGPRs / 27 KB of LDS for the split
// form; the wide form keeps the fp32 tile in LDS for the exact checks).
// (Round 5, for graphs whose launch is one under-filled round of workgroups -- 100 K vertices: 782 workgroups on 256 CUs --
// tiles of 256 edges, R = 1, twice the workgroups: 59.1 us per iteration against 54.5, the fused kernel 32.4 against 28.0.)
//
// The query-cell pre-filter (spring_scan_cells_kernel) serves D <= 3 with up to GH_QC_SMAX queries: one staged group of
// query records and one uint8 index per table entry.  AUTO takes it wherever the thresholds have a launch of their own
// (graphs of more than 2048 fused workgroups); where they are computed inside the fused launch the split-f16 form stays.
// The first workgroup of the query-cell launch can take the thresholds from coarse group minima itself (setup_core.h
// "COARSE FORM", qcell_core.h gh_ct_tau).  Which of these an engine runs: gh_make_step_plan (step_plan.h).

// The copy of the coarse table that the set-up of iteration `iter` fills must be empty: it is, unless a set-up done ahead
// was discarded (other ids, positions set, another threshold form in between) after it had written.
gh_status gh_cmin_claim(gh_engine *h, uint64_t iter) {
    const int p = (int)(iter & 1);
    if (h->cmin_dirty[p])
        GH_HIP(hipMemsetAsync(h->d_cmin.p + (size_t)p * GH_CT_M * (size_t)h->S, 0xFF, sizeof(uint32_t) * GH_CT_M * (size_t)h->S, h->stream));
    h->cmin_dirty[p] = true;
    return GH_OK;
}
namespace {

// Phase A of both fused kernels for one workgroup: spring forces of the vertices v0..v1 -> Fs,
// midpoints of their owned edges -> LDS, and new0 = pos + Fs -> out_new (pt.py:796-799 for every
// vertex the intersection phase does not touch: Fs + 0 == Fs exactly; the few touched vertices are
// redone by stats_fix_kernel).  Returns this thread's column sums of new0 for the fp64 statistics.
// CG: own rows and neighbour rows come from the sector-packed table `cg` (common.h gh_cg_slot) and pos is read only for
// the hub rows' midpoints: the own-row stream then warms the very lines the gathers hit.
template <int D, int LD, int NT, bool LONG, bool CG = false>
__device__ __forceinline__ void gh_phase_a(const float *__restrict__ pos, const int32_t *__restrict__ rowptr,
                                           const int32_t *__restrict__ adj, const int32_t *__restrict__ first_edge,
                                           int v0, int v1, int fe0, int nedges, int64_t row_lo, float L_min, float neg_k,
                                           float *__restrict__ Fs, float *__restrict__ out_new, float *mids,
                                           double (&sx)[LD], double (&sxx)[LD], const gh_long_args &la,
                                           const float *__restrict__ Fpre = nullptr /* hub forces (the Fs array) */,
                                           const float *__restrict__ cg = nullptr) {
    if (!Fpre) Fpre = Fs;
#pragma unroll
    for (int d = 0; d < LD; ++d) { sx[d] = 0.0; sxx[d] = 0.0; }
    for (int i = v0 + threadIdx.x; i < v1; i += NT) {
        const int64_t x = row_lo + i;
        float px[LD], F[LD], nw[LD];
        gh_gather_row<LD, CG>(CG ? cg : pos, x, px);
        // LONG: the graph has hub rows (their forces come from spring_long_kernel); kept out of the
        // common instantiation, where the extra path costs 8 VGPRs and with them a wave of occupancy
        if constexpr (LONG)
            spring_row<D, LD, true, CG>(pos, adj, rowptr[i], rowptr[i + 1], x, px, L_min, neg_k, F, mids, first_edge[i] - fe0,
                                        la, i, Fpre + (int64_t)i * LD, cg);
        else
            spring_pull<D, LD, true, CG>(CG ? cg : pos, adj, rowptr[i], rowptr[i + 1], x, px, L_min, neg_k, F, mids, first_edge[i] - fe0);
        if (Fs) gh_store_row<LD>(Fs, i, F);
#pragma unroll
        for (int d = 0; d < LD; ++d) {
            nw[d] = px[d] + F[d];
            sx[d] += (double)nw[d];
            sxx[d] += (double)nw[d] * (double)nw[d];
        }
        if (out_new) gh_store_row<LD>(out_new, i, nw);
    }
    if constexpr (LONG)
        if (la.n > 0 && la.own_long) gh_long_midpoints<D, LD, NT>(pos, la, fe0, nedges, mids);
}

// Workgroup reduction of the per-thread column sums -> blockstats[entry][blockIdx.x], entry < 2*LD (fixed order).
template <int LD, int NT>
__device__ __forceinline__ void gh_block_stats(const double (&sx)[LD], const double (&sxx)[LD], double *red /* [NT/64][2*LD] */,
                                               double *__restrict__ blockstats, int bx, int nbx, int nrows) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // a wave none of whose threads had a row (a tile of 512 owned edges is ~128 rows for 256 threads) holds zeros: it
    // stores them and skips the 2 LD shuffle trees -- 240 instructions, half of them LDS permutes, per idle wave (round 3:
    // the trees of all four waves were 4 M of the kernel's 42 M VALU instructions and most of its LDS instructions)
    if (w * 64 >= nrows) {
        if (lane < 2 * LD) red[w * 2 * LD + lane] = 0.0;
    } else {
#pragma unroll
        for (int d = 0; d < LD; ++d) {
            const double a = gh_wave_sum(sx[d]), b = gh_wave_sum(sxx[d]);
            if (lane == 0) { red[w * 2 * LD + d] = a; red[w * 2 * LD + LD + d] = b; }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * LD && blockstats) {
        double v = red[threadIdx.x];
#pragma unroll
        for (int ww = 1; ww < NT / 64; ++ww) v += red[ww * 2 * LD + threadIdx.x];
        blockstats[(int64_t)threadIdx.x * nbx + bx] = v;  // [entry][workgroup]: the reducers read contiguously
    }
}


// MFMA form of phase B (D <= 3, 256 threads, tiles of 256*R edges): the pre-filter of scan_core.h
// on v_mfma_f32_32x32x16_f16 with split-f16 operands.  Each wave owns 64*R references of the tile
// as NB = 2R column blocks of 32 whose B operands live in registers for the whole scan; the
// queries stream past as A operands, 32 per MFMA, read from LDS.  A lane owns one reference column
// and 16 query rows of every 32x32 result: a min tree over its 16 accumulators and one compare
// decide whether any of those pairs needs the exact re-check (fp32 fma chain on the fp32 midpoint
// and query kept in LDS -- bit-identical to the VALU form and to the oracle).
// DEFER: the pairs that pass the filter are listed and decided by all threads after the group's last matrix instruction
// (as in spring_scan_mfmaw_kernel) instead of on the spot by the lane that found them.  Pays where a workgroup meets many
// of them -- a graph of 100 K vertices, ~70 per workgroup: 59.4 -> 58.2 us per iteration -- and costs three VGPRs, i.e. a wave
// of occupancy: the launcher takes it for graphs whose workgroups all run at once anyway (1 M vertices with it: 173 -> 189 us).
// CG: phase A reads position rows from the sector-packed table `cg` (gh_phase_a).
template <int D, int R, bool DEFER = false, bool CG = false>
__global__ __launch_bounds__(256) void spring_scan_mfma_kernel(
    const float *__restrict__ pos, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ adj,
    const int32_t *__restrict__ first_edge, const int32_t *__restrict__ own_eids,
    const int32_t *__restrict__ vblock, int64_t row_lo, float L_min, float neg_k, float *__restrict__ Fs,
    float *__restrict__ out_new, double *__restrict__ blockstats, const float *__restrict__ qt,
    const gh_h8 *__restrict__ qA, const int32_t *__restrict__ qexact, int S, uint64_t *__restrict__ cand,
    int32_t *__restrict__ cnt, gh_long_args la, gh_tau_args ta, unsigned long long *__restrict__ stamps,
    const float *__restrict__ cg) {
    constexpr int LD = 4, NT = 256, TILE = NT * R, NB = 2 * R, HITBUF = 512;
    if ((int)blockIdx.x < ta.nblocks) {  // thresholds of this launch (tau_core.h); diagnostic stamps: the last records of the buffer
        gh_tau_produce<NT, 0>(ta, stamps ? stamps + ((int64_t)gridDim.x - 2 * ta.nblocks + GH_STAMP_EXTRA + blockIdx.x) * 8 : nullptr);
        return;
    }
    const bool coh = ta.nblocks > 0;
    const int nbx = (int)gridDim.x - ta.nblocks;
    const int bx = (int)blockIdx.x - ta.nblocks;
#define GH_STAMP(k) do { if (stamps && threadIdx.x == 0 && blockIdx.y == 0) stamps[(int64_t)bx * 8 + (k)] = wall_clock64(); } while (0)
    GH_STAMP(0);
    if (stamps && threadIdx.x == 0) { stamps[(int64_t)bx * 8 + 6] = vblock[bx + 1] - vblock[bx]; stamps[(int64_t)bx * 8 + 7] = first_edge[vblock[bx + 1]] - first_edge[vblock[bx]]; }
    static_assert(D <= 3, "one 16-deep contraction holds three split coordinates");
    __shared__ float4 tile[TILE];                    // fp32 midpoints of the owned edges (x, y, z, 0)
    __shared__ gh_h8 qa[GH_SCAN_QGROUP * 2];         // A rows: [query][half]
    __shared__ float4 qrec[GH_SCAN_QGROUP];          // (q_0, q_1, q_2, tau) for the exact re-check
    __shared__ uint64_t hkey[HITBUF];
    __shared__ int hq[HITBUF];
    __shared__ uint16_t badlist[TILE];               // references outside the f16 range of the filter
    __shared__ uint32_t ids[TILE];                   // edge ids of the tile's references (the exact path must not wait for memory)
    constexpr int PENDCAP = DEFER ? 512 : 1;
    __shared__ uint32_t pend[PENDCAP];   // (query of the group) << 16 | reference
    __shared__ int hcount, nbad, npend;
    float *mids = reinterpret_cast<float *>(tile);

    const int v0 = vblock[bx], v1 = vblock[bx + 1];
    const int fe0 = first_edge[v0];
    const int nedges = first_edge[v1] - fe0;
    if (threadIdx.x == 0) { hcount = 0; nbad = 0; npend = 0; }
    // The tile's edge ids do not depend on the spring phase: fetched now, under its gathers.  (So were the first query
    // group's operand rows while the thresholds had a launch of their own -- measured neutral at 100 K and 1 M vertices,
    // tools/stamp_probe.py: the scan's 8 us per workgroup there are its ~70 divergent hits, not its staging.)
    auto stage_queries = [&](int s_lo, int nq) {
        const int q = threadIdx.x;  // one query per thread: 32 B of A row, 16 B of exact record
        if (q < nq) {
            const float4 *arow = reinterpret_cast<const float4 *>(qA + 2 * (s_lo + q));
            float4 a0, a1, rec;
            gh_ld_f4x3(arow, arow + 1, reinterpret_cast<const float4 *>(qt) + s_lo + q, coh, a0, a1, rec);
            reinterpret_cast<float4 *>(qa)[2 * q] = a0;
            reinterpret_cast<float4 *>(qa)[2 * q + 1] = a1;
            qrec[q] = rec;
        } else {  // padding row: never passes
            const _Float16 z = (_Float16)0.0f;
            qa[2 * q] = (gh_h8){z, z, z, z, z, z, z, z};
            qa[2 * q + 1] = (gh_h8){z, z, z, z, (_Float16)GH_MF_NEVER, z, z, z};
            qrec[q] = make_float4(0.f, 0.f, 0.f, -1.f);
        }
    };
    for (int j = threadIdx.x; j < nedges; j += NT) ids[j] = own_eids ? (uint32_t)own_eids[fe0 + j] : (uint32_t)(fe0 + j);

    __shared__ double red[(NT / 64) * 2 * LD];
    {
        double sx[LD], sxx[LD];
        gh_phase_a<D, LD, NT, true, CG>(pos, rowptr, adj, first_edge, v0, v1, fe0, nedges, row_lo, L_min, neg_k, Fs, out_new, mids, sx, sxx, la,
                                        nullptr, cg);
        GH_STAMP(1);
        gh_block_stats<LD, NT>(sx, sxx, red, blockstats, bx, nbx, v1 - v0);  // contains the barrier that ends phase A
    }
    GH_STAMP(2);

    // B operands of this wave's NB column blocks; a reference outside the f16 range never passes the
    // MFMA filter and is scanned exactly by its lane (half 0) below
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 31, hsel = lane >> 5;
    gh_h8 B[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = w * (64 * R) + b * 32 + col;
        const float4 mv4 = tile[j < nedges ? j : 0];
        const float mv[3] = {mv4.x, mv4.y, mv4.z};
        // out of the f16 range: listed, and scanned exactly by the whole workgroup after each query group
        if (!gh_mf_ref_col(mv, j < nedges, hsel, B[b]) && hsel == 0) badlist[atomicAdd(&nbad, 1)] = (uint16_t)j;
    }

    auto park = [&](int s_lo, int s, int j) {  // exact decision on pair (query s of the group, reference j)
        const float4 qr = qrec[s];
        const float4 mv = tile[j];
        const float q[3] = {qr.x, qr.y, qr.z}, m[3] = {mv.x, mv.y, mv.z};
        float d2 = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float df = q[d] - m[d];
            d2 = fmaf(df, df, d2);
        }
        if (d2 <= qr.w) {
            if (ta.cdist) d2 = gh_aten_cdist<D>(q, m);   // parity mode: the key carries the value the reference ranks
            const uint32_t id = ids[j];
            const int p = atomicAdd(&hcount, 1);
            if (p < HITBUF) { hkey[p] = gh_key(d2, id); hq[p] = s_lo + s; }
            else gh_append_candidate(cand, cnt, s_lo + s, gh_key(d2, id));
        }
    };
    if (ta.nblocks > 0) {  // thresholds of this launch: out by now, as a rule
        if (stamps && threadIdx.x == 0) stamps[(int64_t)bx * 8 + 6] = wall_clock64();
        if (threadIdx.x == 0) gh_tau_wait(ta);
        if (stamps && threadIdx.x == 0) stamps[(int64_t)bx * 8 + 7] = wall_clock64();
        __syncthreads();
    }
    const int nex = (int)gh_ld_u32(qexact, coh);
    GH_STAMP(3);

    for (int s_lo = 0; s_lo < S; s_lo += GH_SCAN_QGROUP) {
        const int nq = min(S - s_lo, GH_SCAN_QGROUP);
        if (s_lo > 0) {
            __syncthreads();  // the previous group's rows (and pair list) are still being read
            if (hcount >= HITBUF / 4) {  // many query groups: the parked hits leave before the buffer fills
                gh_flush_hits<HITBUF, NT>(hkey, hq, &hcount, cand, cnt);
                __syncthreads();
                if (threadIdx.x == 0) hcount = 0;
            }
            if constexpr (DEFER) { if (threadIdx.x == 0) npend = 0; }
        }
        stage_queries(s_lo, nq);
        __syncthreads();   // staged rows, edge ids, the list of out-of-range references: visible to every thread
        const int nqb = (nq + 31) / 32;
        const gh_f16x zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int qb = 0; qb < nqb; ++qb) {
            const gh_h8 a = qa[2 * (qb * 32 + col) + hsel];
            // the MFMA of block b+1 is issued before block b's result is tested: its 32 cycles in the
            // matrix pipe run under the ~10 VALU instructions of the test
            gh_f16x f = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, B[0], zero, 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                gh_f16x fn = zero;
                if (b + 1 < NB) fn = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, B[b + 1], zero, 0, 0, 0);
                // any F <= 0 <=> the smallest of the 16 values read as int32 is <= 0 (sign-magnitude
                // floats order like integers across zero; -0 reads as INT_MIN)
                int mn = min(__float_as_int(f[0]), __float_as_int(f[1]));
#pragma unroll
                for (int i = 2; i < 16; ++i) mn = min(mn, __float_as_int(f[i]));
                asm volatile("" : "+v"(mn));  // opaque: else the compiler drops the tree for 16 tests + branches
                if (mn <= 0) {  // rare: result row (i&3) + 8(i>>2) + 4*half, column = this lane's reference
                    // sign bits of the 16 values, f[0] in bit 15 ... f[15] in bit 0 (a candidate has F < 0:
                    // the slack in C0 and T is twice the error bound), then one exact re-check per set bit
                    uint32_t m = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) m = __builtin_amdgcn_alignbit(m, __float_as_uint(f[i]), 31);
                    const int j = w * (64 * R) + b * 32 + col;
                    if (j < nedges) {
                        while (m) {
                            const int bit = 31 - __builtin_clz(m);
                            m &= ~(1u << bit);
                            const int i = 15 - bit;
                            const int s = qb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hsel;
                            if (s < nq) {
                                if constexpr (DEFER) {
                                    const int p = atomicAdd(&npend, 1);
                                    if (p < PENDCAP) pend[p] = ((uint32_t)s << 16) | (uint32_t)j;
                                    else park(s_lo, s, j);   // list full: decided on the spot
                                } else {
                                    park(s_lo, s, j);
                                }
                            }
                        }
                    }
                }
                f = fn;
            }
        }
        if constexpr (DEFER) {
            __syncthreads();
            for (int p = threadIdx.x, np = min(npend, PENDCAP); p < np; p += NT) park(s_lo, (int)(pend[p] >> 16), (int)(pend[p] & 0xFFFFu));
        }
        // outside the f16 range: exact scan of this group's listed queries over the whole tile ...
        for (int x = 0; x < nex; ++x) {
            const int s = (int)gh_ld_u32(qexact + 1 + x, coh) - s_lo;
            if (s < 0 || s >= nq) continue;
            for (int j = threadIdx.x; j < nedges; j += NT) park(s_lo, s, j);
        }
        // ... and of the tile's out-of-range references against every query of the group: all threads, one
        // pair each (a layout in which a hub has flown off takes thousands of midpoints out of range)
        const int nb_ = nbad;  // complete: the staging barrier of this group came after the B operands were built
        for (int p = threadIdx.x; p < nb_ * nq; p += NT) {
            const int s = p % nq;
            const gh_h8 hi = qa[2 * s + 1];
            if ((float)hi[4] == GH_MF_NEVER) continue;  // a listed query: the loop above has done this pair
            park(s_lo, s, badlist[p / nq]);
        }
    }
    __syncthreads();
    GH_STAMP(4);
    gh_flush_hits<HITBUF, NT>(hkey, hq, &hcount, cand, cnt);
    GH_STAMP(5);
#undef GH_STAMP
}

// Query-cell form of phase B (D <= 3; qcell_core.h).  Workgroup 0 of the launch builds the cell table of the S query
// balls from the thresholds a launch of their own has left in memory, while the others run phase A, and publishes it as
// gh_tau_produce publishes thresholds (write-through stores, the wave waits for them, then the flag -- here the number
// of this launch, so nothing has to zero it).  The waves without rows in phase A wait for the flag and stage the table
// (sc1 loads) and the S query records while the others gather; after phase A each thread takes 2 midpoints of the tile:
// the queries listed in its cell, then the wide ones, each through the exact fp32 test and hit buffer of the MFMA form.
// Same candidates as that form by construction: both keep exactly the pairs with fp32 d2 <= tau (the MFMA filter and
// this table only decide which pairs reach the test).
// rr1m (tools/stamp_probe.py, median workgroup): scan 6.1 -> 3.2 us, operand build / staging 1.2 -> 0.04, lifetime 18.3
// -> 16.1; the gathers of phase A take 8.1 -> 9.1 us, with more workgroups in phase A at a time.  Kernel 129.5 -> 114.1
// us.  88 VGPRs (77 for D = 2), 24.2 KB of LDS: five workgroups per CU, as for the MFMA form (91 VGPRs, 30 KB); six
// would need 80 VGPRs, which the compiler reaches only by spilling (36 bytes per lane; not measured).
// KC > 0: no threshold launch has run.  Workgroup 0 first takes every query's tau from its coarse group minima (thread s:
// gh_ct_tau<KC>, K <= KC keys; setup_core.h "COARSE FORM"), stores it into the query record for the launches behind this
// one, builds the table from the records at hand and publishes the S records behind the table, under the same flag; the
// other workgroups stage the records from there, after the poll, instead of from qt before it.
// CG: phase A reads position rows from the sector-packed table `cg` (gh_phase_a).
template <int D, int KC, bool CG = false>
__global__ __launch_bounds__(256) void spring_scan_cells_kernel(
    const float *__restrict__ pos, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ adj,
    const int32_t *__restrict__ first_edge, const int32_t *__restrict__ own_eids,
    const int32_t *__restrict__ vblock, int64_t row_lo, float L_min, float neg_k, float *__restrict__ Fs,
    float *__restrict__ out_new, double *__restrict__ blockstats, float *__restrict__ qt, int S,
    uint32_t *__restrict__ qcell, unsigned *__restrict__ qc_flag, unsigned epoch, int32_t *__restrict__ wait_failed,
    uint64_t *__restrict__ cand, int32_t *__restrict__ cnt, gh_long_args la, int cdist, unsigned long long *__restrict__ stamps,
    uint32_t *__restrict__ cmin /* KC > 0: this iteration's copy of the coarse table */, int K,
    int32_t *__restrict__ tcount_reset /* KC > 0: the touched-list counter to reset (the threshold launch did), or null */,
    const float *__restrict__ cg) {
    constexpr int LD = 4, NT = 256, R = 2, TILE = NT * R, HITBUF = 512;
    static_assert(D <= 3, "query records of one 16-byte load");
    __shared__ float4 tile[TILE];               // fp32 midpoints of the owned edges (x, y, z, 0)
    __shared__ float4 qrec[GH_QC_SMAX];         // (q_0, q_1, q_2, tau)
    __shared__ uint32_t tab[GH_QC_TAB_WORDS];   // the cell table (qcell_core.h)
    __shared__ uint64_t hkey[HITBUF];
    __shared__ int hq[HITBUF];
    __shared__ uint32_t ids[TILE];
    __shared__ int hcount;
    if (blockIdx.x == 0) {   // the table of this launch (scratch counters in the hit buffer)
        // diagnostic stamps of this workgroup: the last record of the buffer (start, thresholds, table built, flag set)
        unsigned long long *st0 = stamps && threadIdx.x == 0 ? stamps + ((int64_t)gridDim.x - 1 + GH_STAMP_EXTRA - 1) * 8 : nullptr;
        if (st0) st0[0] = wall_clock64();
        float4 r = make_float4(0.f, 0.f, 0.f, -1.f);
        if ((int)threadIdx.x < S) r = reinterpret_cast<const float4 *>(qt)[threadIdx.x];
        unsigned long long *stb = st0 ? st0 - 8 : nullptr;   // (the record before: the stages of the table build)
        if constexpr (KC > 0) {
            // up to a dozen keys in three dimensions the batch is the whole row -- one memory round trip (qcell_core.h) -- at 90
            // VGPRs instead of 88, still five workgroups per CU; the two-dimensional kernel would go from 77 to 88 and from
            // six to five, the 32-key one past its budget too
            constexpr int B = KC <= 12 ? (D == 3 ? GH_CT_M : 16) : (D == 3 ? 8 : 4);
            // first of all: this workgroup starts before the gathers of the others fill the memory system's queues
            if (threadIdx.x == 0 && tcount_reset) *tcount_reset = 0;
            if ((int)threadIdx.x < S) {
                r.w = gh_ct_tau<KC, B>(cmin, threadIdx.x, (uint32_t)S, K);
                qt[threadIdx.x * 4 + 3] = r.w;   // read by the launches behind this one (cdist.hip)
            }
            if (st0) st0[1] = wall_clock64();
            gh_qc_frame<D, NT>(r, S, tab, qrec, reinterpret_cast<uint32_t *>(hkey), stb);
            gh_qc_fill<D, NT>(r, S, tab, qrec, reinterpret_cast<uint32_t *>(hkey), stb);
        } else {
            if (st0) st0[1] = wall_clock64();
            gh_qc_build<D, NT>(r, S, tab, qrec, reinterpret_cast<uint32_t *>(hkey), stb);
        }
        if (st0) st0[2] = wall_clock64();
        for (int i = threadIdx.x; i < GH_QC_TAB_WORDS; i += NT)
            __hip_atomic_store(qcell + i, tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (KC > 0) {
            if ((int)threadIdx.x < S) {
                uint32_t *dst = qcell + GH_QC_OFF_REC + 4 * threadIdx.x;
                __hip_atomic_store(dst + 0, __float_as_uint(r.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(dst + 1, __float_as_uint(r.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(dst + 2, __float_as_uint(r.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(dst + 3, __float_as_uint(r.w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's write-through stores have left ...
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(qc_flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... before the flag
        if (st0) st0[3] = wall_clock64();
        return;
    }
    const int nbx = (int)gridDim.x - 1;
    const int bx = (int)blockIdx.x - 1;
#define GH_STAMP(k) do { if (stamps && threadIdx.x == 0) stamps[(int64_t)bx * 8 + (k)] = wall_clock64(); } while (0)
    GH_STAMP(0);
    if (stamps && threadIdx.x == 0) { stamps[(int64_t)bx * 8 + 6] = vblock[bx + 1] - vblock[bx]; stamps[(int64_t)bx * 8 + 7] = first_edge[vblock[bx + 1]] - first_edge[vblock[bx]]; }
    float *mids = reinterpret_cast<float *>(tile);
    const int v0 = vblock[bx], v1 = vblock[bx + 1];
    const int fe0 = first_edge[v0];
    const int nedges = first_edge[v1] - fe0;
    if (threadIdx.x == 0) hcount = 0;
    for (int j = threadIdx.x; j < nedges; j += NT) ids[j] = own_eids ? (uint32_t)own_eids[fe0 + j] : (uint32_t)(fe0 + j);

    // Staging: the query records (written by the threshold launch before this one: plain loads), then -- once workgroup 0
    // has published it: a wave-wide poll, one request per wave -- the table (sc1 loads).  A tile of 512 owned edges is ~128
    // rows for 256 threads, so as a rule waves 2 and 3 have nothing to do in phase A: they stage while the others gather,
    // and the barrier in gh_block_stats publishes it.  A workgroup whose rows take every wave stages after phase A.
    const int t_idle = min(NT, (v1 - v0 + 63) / 64 * 64);   // first thread of the first wave without rows
    auto stage = [&](int t0) {   // by threads t0 .. NT - 1
        if constexpr (KC == 0)
            for (int i = (int)threadIdx.x - t0; i < S; i += NT - t0) qrec[i] = reinterpret_cast<const float4 *>(qt)[i];
        unsigned spins = 0;
        while ((int)(__hip_atomic_load(qc_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - epoch) < 0) {
            __builtin_amdgcn_s_sleep(32);
            if (++spins > (1u << 20)) { *wait_failed = 1; break; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // orders the loads below after the poll; no cache invalidate
        for (int i = (int)threadIdx.x - t0; i < GH_QC_TAB_WORDS / 4; i += NT - t0)
            reinterpret_cast<float4 *>(tab)[i] = gh_ld_f4(reinterpret_cast<const float4 *>(qcell) + i, true);
        if constexpr (KC > 0)   // the records with this launch's thresholds, published behind the table
            for (int i = (int)threadIdx.x - t0; i < S; i += NT - t0)
                qrec[i] = gh_ld_f4(reinterpret_cast<const float4 *>(qcell + GH_QC_OFF_REC) + i, true);
    };
    if (t_idle < NT && (int)threadIdx.x >= t_idle) stage(t_idle);

    __shared__ double red[(NT / 64) * 2 * LD];
    {
        double sx[LD], sxx[LD];
        gh_phase_a<D, LD, NT, true, CG>(pos, rowptr, adj, first_edge, v0, v1, fe0, nedges, row_lo, L_min, neg_k, Fs, out_new, mids, sx, sxx, la,
                                        nullptr, cg);
        GH_STAMP(1);
        gh_block_stats<LD, NT>(sx, sxx, red, blockstats, bx, nbx, v1 - v0);  // contains the barrier that ends phase A
    }
    GH_STAMP(2);
    if (t_idle == NT) {
        stage(0);
        __syncthreads();
    }
    GH_STAMP(3);

    const float *bnd = reinterpret_cast<const float *>(tab + GH_QC_OFF_B);
    const uint16_t *ptr = reinterpret_cast<const uint16_t *>(tab + GH_QC_OFF_PTR);
    const uint8_t *ent = reinterpret_cast<const uint8_t *>(tab + GH_QC_OFF_ENT);
    const uint8_t *wide = reinterpret_cast<const uint8_t *>(tab + GH_QC_OFF_WIDE);
    const int nwide = (int)tab[GH_QC_OFF_NWIDE];
    auto park = [&](int s, const float4 qr, int j, const float (&m)[3]) {  // exact decision on pair (query s = qr, reference j)
        const float q[3] = {qr.x, qr.y, qr.z};
        float d2 = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float df = q[d] - m[d];
            d2 = fmaf(df, df, d2);
        }
        if (d2 <= qr.w) {
            if (cdist) d2 = gh_aten_cdist<D>(q, m);   // parity mode: the key carries the value the reference ranks
            const uint32_t id = ids[j];
            const int p = atomicAdd(&hcount, 1);
            if (p < HITBUF) { hkey[p] = gh_key(d2, id); hq[p] = s; }
            else gh_append_candidate(cand, cnt, s, gh_key(d2, id));
        }
    };
    // A thread's tests: the queries listed in the cells of its two midpoints, then the wide ones against both.  U entries
    // at a time, their index and record loads issued back to back: the lists are a handful of entries each (rr1m: ~9
    // tests per midpoint), so the loop is bound by dependent LDS round trips, not by issue -- one entry at a time the
    // scan took 7.2 us of a workgroup's lifetime against the MFMA form's 6.2.
    constexpr int U = 4;
    float m[R][3];
    int e[R], e1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = (int)threadIdx.x + r * NT;
        const float4 mv = tile[j < nedges ? j : 0];
        m[r][0] = mv.x; m[r][1] = mv.y; m[r][2] = mv.z;
        int c = gh_qc_axis_cell(bnd, m[r][0]) + GH_QC_G * gh_qc_axis_cell(bnd + 8, m[r][1]);
        if constexpr (D == 3) c += GH_QC_G * GH_QC_G * gh_qc_axis_cell(bnd + 16, m[r][2]);
        e[r] = j < nedges ? ptr[c] : 0;
        e1[r] = j < nedges ? ptr[c + 1] : 0;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = (int)threadIdx.x + r * NT;
        for (int b = e[r]; b < e1[r]; b += U) {
            int s[U];
            float4 qr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = ent[min(b + u, e1[r] - 1)];
#pragma unroll
            for (int u = 0; u < U; ++u) qr[u] = qrec[s[u]];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (b + u < e1[r]) park(s[u], qr[u], j, m[r]);
        }
    }
    for (int b = 0; b < nwide; b += U) {
        int s[U];
        float4 qr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = wide[min(b + u, nwide - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) qr[u] = qrec[s[u]];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = (int)threadIdx.x + r * NT;
            if (j < nedges) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (b + u < nwide) park(s[u], qr[u], j, m[r]);
            }
        }
    }
    __syncthreads();
    GH_STAMP(4);
    gh_flush_hits<HITBUF, NT>(hkey, hq, &hcount, cand, cnt);
    GH_STAMP(5);
#undef GH_STAMP
}

// Wide rows (5 <= D <= 16) with the pre-filter on the matrix pipe (scan_core.h "Wide rows"): phase A as in
// spring_scan_kernel, phase B as in spring_scan_mfma_kernel with 16 * KB deep contractions -- each wave owns 4 column
// blocks of 32 references whose f16 operands stay in registers, the queries stream past as A operands from LDS, a lane
// owns one reference column and 16 query rows of every 32x32 result; the fp32 tile and query records stay in LDS for
// the exact re-check of the few pairs that pass.  Tile = 512 owned edges, 256 threads.
// Packed fp32 VALU needs D/2 instructions per pair and lane; this form one (two) matrix instructions per 1024 pairs plus
// the same ~10 VALU instructions to test them.
template <int D, int LD, bool LONG>
__global__ __launch_bounds__(256) void spring_scan_mfmaw_kernel(
    const float *__restrict__ pos, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ adj,
    const int32_t *__restrict__ first_edge, const int32_t *__restrict__ own_eids,
    const int32_t *__restrict__ vblock, int64_t row_lo, float L_min, float neg_k, float *__restrict__ Fs,
    float *__restrict__ out_new, double *__restrict__ blockstats, const float *__restrict__ qt,
    const float *__restrict__ qscan, int S,
    uint64_t *__restrict__ cand, int32_t *__restrict__ cnt, gh_long_args la, gh_tau_args ta,
    unsigned long long *__restrict__ stamps) {
    constexpr int NT = 256, R = 2, TILE = NT * R, NB = 2 * R;
    constexpr int HITBUF = LD == 16 ? 256 : 512;   // (16-float rows: two workgroups per CU must fit 160 KB of LDS)
    constexpr int KB = D <= 10 ? 1 : 2;
    constexpr int QS = LD + 4, QT = LD;
    if ((int)blockIdx.x < ta.nblocks) {
        if (blockIdx.y == 0) gh_tau_produce<NT, -1>(ta, stamps ? stamps + ((int64_t)gridDim.x - 2 * ta.nblocks + GH_STAMP_EXTRA + blockIdx.x) * 8 : nullptr);
        return;
    }
    const bool coh = ta.nblocks > 0;
    const int nbx = (int)gridDim.x - ta.nblocks;
    const int bx = (int)blockIdx.x - ta.nblocks;
#define GH_STAMP(k) do { if (stamps && threadIdx.x == 0 && blockIdx.y == 0) stamps[(int64_t)bx * 8 + (k)] = wall_clock64(); } while (0)
    GH_STAMP(0);
    __shared__ float4 tile[TILE * LD / 4];                 // fp32 midpoints of the owned edges
    __shared__ gh_h8 qa[GH_SCAN_QGROUP * KB * 2];          // A rows: [query][block of 16][half]
    __shared__ float4 qsh[(GH_SCAN_QGROUP + 1) * (QS / 4)]; // (-2q, t) records: the exact re-check takes q from them
    __shared__ float taush[GH_SCAN_QGROUP];
    __shared__ uint64_t hkey[HITBUF];
    __shared__ int hq[HITBUF];
    __shared__ uint16_t badlist[TILE];
    __shared__ uint32_t ids[TILE];
    __shared__ uint16_t exq[GH_SCAN_QGROUP];               // queries of the group outside the f16 range
    // pairs that passed the filter, (query of the group) << 16 | reference: listed by the lane that found them and decided
    // exactly by ALL threads after the group's last matrix instruction -- inline, each pair is a divergent detour of a
    // D-step chain and two LDS row reads for one lane of a wave, and this form lets ~3x the necessary pairs through
    // (D = 6 at 1 M vertices: 277 -> 266 us per iteration; the split form of D <= 3 keeps the inline check: there the list
    // cost it three VGPRs -- a wave of occupancy -- for a dozen pairs per workgroup: 173 -> 189 us)
    constexpr int PENDCAP = 512;
    __shared__ uint32_t pend[PENDCAP];
    __shared__ int hcount, nbad, nexq, npend;
    float *mids = reinterpret_cast<float *>(tile);

    const int v0 = vblock[bx], v1 = vblock[bx + 1];
    const int fe0 = first_edge[v0];
    const int nedges = first_edge[v1] - fe0;
    if (threadIdx.x == 0) { hcount = 0; nbad = 0; nexq = 0; npend = 0; }
    for (int j = threadIdx.x; j < nedges; j += NT) ids[j] = own_eids ? (uint32_t)own_eids[fe0 + j] : (uint32_t)(fe0 + j);

    // ---- phase A (every query slice redoes it for its tile, slice 0 alone stores its results)
    // (the reduction scratch lives in the hit buffer, idle until the scan: two workgroups of 16-float rows fit the CU's
    // 160 KB of LDS with 3 KB to spare instead of 0.8)
    static_assert(sizeof(double) * (NT / 64) * 2 * LD <= sizeof(uint64_t) * HITBUF, "reduction scratch must fit the hit buffer");
    double *red = reinterpret_cast<double *>(hkey);
    {
        double sx[LD], sxx[LD];
        const bool store = blockIdx.y == 0;
        gh_phase_a<D, LD, NT, LONG>(pos, rowptr, adj, first_edge, v0, v1, fe0, nedges, row_lo, L_min, neg_k, store ? Fs : nullptr,
                                    store ? out_new : nullptr, mids, sx, sxx, la, Fs);
        GH_STAMP(1);
        gh_block_stats<LD, NT>(sx, sxx, red, store ? blockstats : nullptr, bx, nbx, v1 - v0);  // contains the barrier that ends phase A
    }
    GH_STAMP(2);

    // ---- phase B: operands of this wave's column blocks
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 31, hsel = lane >> 5;
    gh_h8 B[NB][KB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = w * (64 * R) + b * 32 + col;
        float mv[LD];
        gh_load_row<LD>(mids, j < nedges ? j : 0, mv);
        if (!gh_mfw_ref_col<D, KB>(mv, j < nedges, hsel, B[b]) && hsel == 0) badlist[atomicAdd(&nbad, 1)] = (uint16_t)j;
    }

    auto park = [&](int s_lo, int s, int j) {  // exact decision on pair (query s of the group, reference j)
        const float *qv = reinterpret_cast<const float *>(qsh) + s * QS;   // (-2q_0 .. -2q_{D-1}, .., t)
        float mv[LD];
        gh_load_row<LD>(mids, j, mv);
        float d2 = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float df = -0.5f * qv[d] - mv[d];   // the record holds -2q: exact both ways
            d2 = fmaf(df, df, d2);
        }
        if (d2 <= taush[s]) {
            if (ta.cdist) {   // parity mode: the key carries the value the reference ranks
                float q[D];
#pragma unroll
                for (int d = 0; d < D; ++d) q[d] = -0.5f * qv[d];
                d2 = gh_aten_cdist<D>(q, mv);
            }
            const uint32_t id = ids[j];
            const int p = atomicAdd(&hcount, 1);
            if (p < HITBUF) { hkey[p] = gh_key(d2, id); hq[p] = s_lo + s; }
            else gh_append_candidate(cand, cnt, s_lo + s, gh_key(d2, id));
        }
    };
    if (stamps && ta.nblocks > 0 && threadIdx.x == 0 && blockIdx.y == 0) stamps[(int64_t)bx * 8 + 6] = wall_clock64();
    if (ta.nblocks > 0 && threadIdx.x == 0) gh_tau_wait(ta);  // thresholds of this launch: out by now, as a rule
    if (stamps && ta.nblocks > 0 && threadIdx.x == 0 && blockIdx.y == 0) stamps[(int64_t)bx * 8 + 7] = wall_clock64();
    __syncthreads();
    GH_STAMP(3);

    const int per = (S + (int)gridDim.y - 1) / (int)gridDim.y;
    const int s_begin = (int)blockIdx.y * per, s_end = min(S, s_begin + per);
    const gh_f16x zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s_lo = s_begin; s_lo < s_end; s_lo += GH_SCAN_QGROUP) {
        const int nq = min(s_end - s_lo, GH_SCAN_QGROUP);
        if (s_lo > s_begin) {
            __syncthreads();  // the previous group's rows and list are still being read
            const bool flush = hcount >= HITBUF / 4;   // many query groups: the parked hits leave before the buffer fills
            if (flush) gh_flush_hits<HITBUF, NT>(hkey, hq, &hcount, cand, cnt);
            __syncthreads();
            if (threadIdx.x == 0) { nexq = 0; npend = 0; if (flush) hcount = 0; }
            __syncthreads();
        }
        gh_stage_queries<QS, QT, NT>(qscan, qt, s_lo, nq, qsh, taush, coh);
        {
            // one query per thread: its A row is BUILT here from the query record and the threshold (80 instructions per
            // group and thread) -- the threshold kernel then carries no operand-row code for this form, which as a launch of
            // its own cost it 15 - 25 us (tau_core.h), and a query outside the f16 range goes on a list of this workgroup
            const int q = threadIdx.x;
            _Float16 row[16 * KB];
            bool ok = true;
            if (q < nq) {
                const float4 *src = reinterpret_cast<const float4 *>(qscan) + (int64_t)(s_lo + q) * (QS / 4);
                float qv[16];
#pragma unroll
                for (int d = 0; d < 16; ++d) qv[d] = 0.0f;
#pragma unroll
                for (int i = 0; i < LD / 4; ++i) {
                    const float4 v = gh_ld_f4(src + i, coh);   // (-2q_0 ..): the record holds -2q, exact both ways
                    qv[4 * i] = -0.5f * v.x; qv[4 * i + 1] = -0.5f * v.y; qv[4 * i + 2] = -0.5f * v.z; qv[4 * i + 3] = -0.5f * v.w;
                }
                const float tau = gh_ld_f32(qt + (int64_t)(s_lo + q) * QS + QT, coh);
                ok = gh_mfw_query_row<KB>(qv, tau, row);
                if (!ok) exq[atomicAdd(&nexq, 1)] = (uint16_t)q;
            } else {  // padding row: never passes
#pragma unroll
                for (int k = 0; k < 16 * KB; ++k) row[k] = (_Float16)0.0f;
                row[gh_mfw<KB>::base + 3] = (_Float16)GH_MF_NEVER;
            }
#pragma unroll
            for (int i = 0; i < 2 * KB; ++i) {
                gh_h8 hv;
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = row[i * 8 + e];
                qa[q * (2 * KB) + i] = hv;
            }
        }
        __syncthreads();   // staged rows, edge ids, the list of out-of-range references: visible to every thread
        const int nqb = (nq + 31) / 32;
        for (int qb = 0; qb < nqb; ++qb) {
            gh_h8 a[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) a[kb] = qa[((qb * 32 + col) * KB + kb) * 2 + hsel];
            auto tile_of = [&](int b) {
                gh_f16x f = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], B[b][0], zero, 0, 0, 0);
                if constexpr (KB == 2) f = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], B[b][1], f, 0, 0, 0);
                return f;
            };
            gh_f16x f = tile_of(0);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                gh_f16x fn = zero;
                if (b + 1 < NB) fn = tile_of(b + 1);   // in the matrix pipe while block b is tested
                int mn = min(__float_as_int(f[0]), __float_as_int(f[1]));
#pragma unroll
                for (int i = 2; i < 16; ++i) mn = min(mn, __float_as_int(f[i]));
                asm volatile("" : "+v"(mn));
                if (mn <= 0) {  // rare: result row (i&3) + 8(i>>2) + 4*half, column = this lane's reference
                    uint32_t m = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) m = __builtin_amdgcn_alignbit(m, __float_as_uint(f[i]), 31);
                    const int j = w * (64 * R) + b * 32 + col;
                    if (j < nedges) {
                        while (m) {
                            const int bit = 31 - __builtin_clz(m);
                            m &= ~(1u << bit);
                            const int i = 15 - bit;
                            const int s = qb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hsel;
                            if (s < nq) {
                                const int p = atomicAdd(&npend, 1);
                                if (p < PENDCAP) pend[p] = ((uint32_t)s << 16) | (uint32_t)j;
                                else park(s_lo, s, j);   // list full: decided on the spot
                            }
                        }
                    }
                }
                f = fn;
            }
        }
        __syncthreads();
        for (int p = threadIdx.x, np = min(npend, PENDCAP); p < np; p += NT) park(s_lo, (int)(pend[p] >> 16), (int)(pend[p] & 0xFFFFu));
        // outside the f16 range: exact scan of this group's listed queries over the whole tile ...
        const int nex = nexq;   // complete: the staging barrier of this group came after the rows were built
        for (int x = 0; x < nex; ++x) {
            const int s = exq[x];
            for (int j = threadIdx.x; j < nedges; j += NT) park(s_lo, s, j);
        }
        // ... and of the tile's out-of-range references against every query of the group
        const int nb_ = nbad;
        for (int p = threadIdx.x; p < nb_ * nq; p += NT) {
            const int s = p % nq;
            const gh_h8 tv = qa[(s * KB + (gh_mfw<KB>::base + 3) / 16) * 2 + ((gh_mfw<KB>::base + 3) % 16) / 8];
            if ((float)tv[(gh_mfw<KB>::base + 3) % 8] == GH_MF_NEVER) continue;  // a listed query: the loop above has done this pair
            park(s_lo, s, badlist[p / nq]);
        }
    }
    __syncthreads();
    GH_STAMP(4);
    gh_flush_hits<HITBUF, NT>(hkey, hq, &hcount, cand, cnt);
    GH_STAMP(5);
#undef GH_STAMP
}

// The thresholds of this iteration: computed by the first workgroups of the fused launch itself (GH_TAUF_EMBEDDED), or
// already in place (knn_tau_kernel ran; nblocks = 0).
static unsigned fused_grid(const gh_engine *h, const gh_tau_args &ta) {
    return (unsigned)(h->n_vblocks + ta.nblocks);
}
gh_tau_args fused_tau_args(gh_engine *h, int nt) {
    gh_tau_args ta{};
    ta.cdist = h->cdist ? 1 : 0;
    if (h->plan.tau != GH_TAUF_EMBEDDED) return ta;
    ta = gh_make_tau_args(h);
    ta.cdist = h->cdist ? 1 : 0;
    ta.flag = h->d_tau_flag.p;        // zeroed by this iteration's set-up (setup_core.h), S once the producers are through
    ta.target = (unsigned)h->S;
    ta.nblocks = gh_tau_blocks((int)h->S, nt);
    ta.wait_failed = h->d_wait_failed.p;
    return ta;
}

// The sector-packed table serves this launch: the plan asks for it and its rows are those of d_pos (engine.h
// gh_step_compact_valid).  Else the padded instantiation -- never a packing launch.
static bool fused_compact(const gh_engine *h) { return h->plan.compact_gather && h->step.compact_valid && h->d_cg.p; }

template <int D, int R, bool DEFER, bool CG>
void launch_mfma_c(gh_engine *h) {
    const gh_tau_args ta = fused_tau_args(h, 256);
    spring_scan_mfma_kernel<D, R, DEFER, CG><<<dim3(fused_grid(h, ta)), dim3(256), 0, h->stream>>>(
        h->d_pos.p, h->d_rowptr.p, h->d_adj.p, h->d_first_edge.p, h->d_own_eids.p, h->d_vblock.p, h->part.row_lo, h->prm.L_min,
        -h->prm.k_attr, h->d_Fs.p, h->d_new, h->d_blockstats.p, h->d_q.p, reinterpret_cast<const gh_h8 *>(h->d_qA.p),
        h->d_qexact.p, (int)h->S, h->d_cand.p, h->d_cnt.p, gh_make_long_args(h, true), ta, h->d_stamps.p, h->d_cg.p);
}
template <int D, int R, bool DEFER>
void launch_mfma_d(gh_engine *h) {
    if constexpr (D == 3) {
        if (fused_compact(h)) { ++h->compact_launches; return launch_mfma_c<D, R, DEFER, true>(h); }
    }
    launch_mfma_c<D, R, DEFER, false>(h);
}
template <int D, int KC, bool CG>
void launch_cells_c(gh_engine *h) {
    if (++h->qc_epoch == 0) h->qc_epoch = 1;   // (0 is the flag's value before the first launch)
    const int p = (int)(h->iter & 1);   // the copy this iteration's set-up filled (gh_make_setup_args)
    spring_scan_cells_kernel<D, KC, CG><<<dim3((unsigned)h->n_vblocks + 1), dim3(256), 0, h->stream>>>(
        h->d_pos.p, h->d_rowptr.p, h->d_adj.p, h->d_first_edge.p, h->d_own_eids.p, h->d_vblock.p, h->part.row_lo, h->prm.L_min,
        -h->prm.k_attr, h->d_Fs.p, h->d_new, h->d_blockstats.p, h->d_q.p, (int)h->S, h->d_qcell.p, h->d_qc_flag.p, h->qc_epoch,
        h->d_wait_failed.p, h->d_cand.p, h->d_cnt.p, gh_make_long_args(h, true), h->cdist ? 1 : 0, h->d_stamps.p,
        KC > 0 ? h->d_cmin.p + (size_t)p * GH_CT_M * (size_t)h->S : nullptr, h->Ksel,
        KC > 0 && h->step.tcount_reset_pending ? h->d_tcount.p : nullptr, h->d_cg.p);
    if (KC > 0) gh_cmin_release(h, h->iter);
}
template <int D, int KC>
void launch_cells_k(gh_engine *h) {
    if constexpr (D == 3) {
        if (fused_compact(h)) { ++h->compact_launches; return launch_cells_c<D, KC, true>(h); }
    }
    launch_cells_c<D, KC, false>(h);
}
// The thresholds: in memory (a launch of their own has run), or taken by workgroup 0 from the coarse table -- the usual
// dozen keys in as many registers per thread, up to GH_CT_KMAX in a kernel of its own.
template <int D>
void launch_cells(gh_engine *h) {
    static_assert(GH_CT_KMAX == 32, "the instantiations below");
    if (h->plan.tau != GH_TAUF_COARSE) launch_cells_k<D, 0>(h);
    else if (h->Ksel <= 12) launch_cells_k<D, 12>(h);
    else launch_cells_k<D, 32>(h);
}
template <int D, int R>
void launch_mfma(gh_engine *h) {
    if (R == 2 && h->n_vblocks <= 2048) launch_mfma_d<D, R, (R == 2)>(h);   // one round of workgroups: occupancy does not matter
    else launch_mfma_d<D, R, false>(h);
}

template <int D, int LD, bool LONG>
void launch_mfmaw_l(gh_engine *h) {
    // few workgroups (a small graph with wide rows): the queries in slices over blockIdx.y, as many as still run all at once
    unsigned ny = 1;
    if (h->n_vblocks < 384) {
        static int resident = 0;  // per instantiation
        if (resident == 0) {
            int occ = 0, cus = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, spring_scan_mfmaw_kernel<D, LD, LONG>, 256, 0) != hipSuccess) occ = 1;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 256;
            resident = (occ > 0 ? occ : 1) * (cus > 0 ? cus : 256);
        }
        ny = (unsigned)(resident / (h->n_vblocks > 0 ? h->n_vblocks : 1));
        if (ny > 4) ny = 4;
        if (ny < 1) ny = 1;
        if ((int64_t)ny * 64 > h->S) ny = 1;
    }
    const gh_tau_args ta = fused_tau_args(h, 256);
    spring_scan_mfmaw_kernel<D, LD, LONG><<<dim3(fused_grid(h, ta), ny), dim3(256), 0, h->stream>>>(
        h->d_pos.p, h->d_rowptr.p, h->d_adj.p, h->d_first_edge.p, h->d_own_eids.p, h->d_vblock.p, h->part.row_lo, h->prm.L_min, -h->prm.k_attr,
        h->d_Fs.p, h->d_new, h->d_blockstats.p, h->d_q.p, h->d_qscan.p, (int)h->S,
        h->d_cand.p, h->d_cnt.p, gh_make_long_args(h, true), ta, h->d_stamps.p);
}
template <int D, int LD>
void launch_mfmaw(gh_engine *h) {
    if (gh_make_long_args(h).n > 0) launch_mfmaw_l<D, LD, true>(h);
    else launch_mfmaw_l<D, LD, false>(h);
}

}  // namespace

gh_status gh_launch_spring_scan(gh_engine *h) {
    if (h->n_vblocks == 0) return GH_OK;
    GH_TRY_ST(gh_launch_spring_long(h, h->d_Fs.p, 0));  // hubs first: their rows' forces are read back in phase A
    gh_scope t(h, "spring_scan");
    bool launched = false;
    switch (h->plan.prefilter) {
    case GH_PRE_WIDE_F16:   // 4..16 components
        launched = gh_dispatch_dim(h->D, [&](auto d, auto ld) {
            if constexpr (d() > 3) launch_mfmaw<d(), ld()>(h);
        });
        break;
    case GH_PRE_CELLS:
        launched = gh_dispatch_value<2, 3>(h->D, [&](auto d) { launch_cells<d()>(h); });
        break;
    case GH_PRE_SPLIT_F16:
        launched = gh_dispatch_value<2, 3>(h->D, [&](auto d) { launch_mfma<d(), GH_FUSED_R>(h); });
        break;
    case GH_PRE_NONE:
        break;
    }
    if (!launched) {   // unreachable: fused_scan needs gh_dim_templated(D) (graph_plan.hip), gh_plan_mfma() a row stride of 4, 8 or 16
        h->err = "fused spring+scan launched for an unsupported dimension";
        return GH_ERR_RUNTIME;
    }
    GH_LAUNCH_CHECK();
    gh_step_new0_ready(h);  // d_new = pos + Fs and d_blockstats[n_vblocks] are in place
    return GH_OK;
}
