// The step plan (graphem-rapids_amd/csrc/step_plan.h) as a stand-alone host program:
//
//     g++ -std=c++17 -O2 -Wall -Werror tools/step_plan_host_check.cpp -o step_plan_host_check && ./step_plan_host_check
//
// The oracle below is a frozen restatement of the predicate chains the plan replaced, as they stood in api.hip, knn.hip,
// grid_core.h, ivf.hip, fused.hip, forces.hip and cdist.hip before it (names kept), over the same plain inputs.  The sweep
// asserts that every field of the plan is what those chains imply, plus the structural facts the callers rely on, and names
// the benchmark's workloads as examples.  Exit status 0: every check held (tests/test_step_plan_host.py).
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "../graphem-rapids_amd/csrc/dispatch.h"    // gh_ld
#include "../graphem-rapids_amd/csrc/step_plan.h"

static long failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { if (++failures <= 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); } } while (0)

// ---- the oracle: the engine members the old predicates read, and the predicates ----------------------------------------
namespace old {
struct engine {
    gh_plan_input in;          // the sizes (the old code read them off gh_engine)
    int scan_filter, coarse_mode;
    bool tau_embedded_plan, opt_no_presetup;
    int64_t thr_stride, thr_M1;
    bool qcells, tau_embedded, coarse_tau;
};
bool gh_knn_scan_path(const engine &h) {
    return h.in.own_count >= 16384 && h.in.LD <= 16 && h.in.D >= 2 && h.in.Ksel <= 128 && h.in.S <= 0x7FFFFFFF;
}
bool gh_grid_path(const engine &h) { return h.in.knn_method == GH_KNN_GRID && h.in.D >= 2 && h.in.D <= 3 && gh_knn_scan_path(h); }
bool gh_ivf_path(const engine &h) {
    return h.in.knn_method == GH_KNN_IVF && !h.in.cdist && h.in.D >= 2 && h.in.LD <= 16 && gh_knn_scan_path(h) &&
           h.in.own_count >= 64 * 64 && h.in.own_count < ((int64_t)1 << 31) - (int64_t)2048 * 512;
}
bool fused_mfma(int LD, int D) { return D <= 16 && (LD == 4 || LD == 8 || LD == 16); }
bool gh_fused_uses_mfma(const engine &h) { return h.in.fused_scan && fused_mfma(h.in.LD, h.in.D); }
int gh_fused_mfma_kb(const engine &h) { return h.in.fused_scan && !h.qcells ? (fused_mfma(h.in.LD, h.in.D) && h.in.D <= 3 ? 0 : -1) : -1; }
bool gh_fused_cells_ok(const engine &h) {
    return h.in.fused_scan && fused_mfma(h.in.LD, h.in.D) && h.in.D <= 3 && h.in.S >= 1 && h.in.S <= 256;
}
bool gh_coarse_tau_ok(const engine &h) { return gh_fused_cells_ok(h) && h.thr_M1 > 0 && h.in.rows == h.in.n && h.in.Ksel <= 32; }
void gh_choose_scan_filter(engine &h) {
    const bool want = h.scan_filter == GH_FILTER_CELLS || (h.scan_filter == GH_FILTER_AUTO && !h.tau_embedded_plan);
    h.qcells = want && gh_fused_cells_ok(h);
    h.tau_embedded = h.tau_embedded_plan && !h.qcells;
    const bool want_coarse = h.coarse_mode == GH_COARSE_ON || (h.coarse_mode == GH_COARSE_AUTO && h.in.D == 3 && h.in.Ksel <= 12);
    h.coarse_tau = h.qcells && want_coarse && gh_coarse_tau_ok(h);
}
// (S = 0 made both quotients infinite; the conversions came to the most negative integer and the result to 2: stated here)
int64_t subset_stride(int64_t Mtot, int K, int64_t S, int tile, bool mfma) {
    if (S == 0) return 2;
    int64_t r = (int64_t)std::sqrt((mfma ? 3.0 : 2.0) * (double)Mtot / ((double)(S < 256 ? S : 256) * K));
    const int64_t by_list = 4096 / K;
    if (r > by_list) r = by_list;
    if (r > 256) r = 256;
    const int64_t by_hits = (int64_t)(300.0 * (double)Mtot / ((double)(S < 256 ? S : 256) * K * tile));
    if (r > by_hits) r = by_hits;
    if (r < 2) r = 2;
    while (r > 2 && Mtot / r < 8 * (int64_t)K * 64) r /= 2;
    return r;
}
void gh_choose_threshold_subset(engine &h) {
    const bool scan = gh_knn_scan_path(h) && !gh_grid_path(h) && !gh_ivf_path(h);
    h.thr_stride = scan ? subset_stride(h.in.own_count, h.in.Ksel, h.in.S, 512, gh_fused_uses_mfma(h)) : 1;
    h.thr_M1 = scan ? (h.in.own_count + h.thr_stride - 1) / h.thr_stride : 0;
}
// step_begin_launches (api.hip), as the search it ends in
gh_search search(const engine &h) {
    if (h.in.S == 0 || h.in.k == 0) return GH_SEARCH_NONE;
    if (gh_grid_path(h)) return GH_SEARCH_GRID;
    if (gh_ivf_path(h)) return GH_SEARCH_IVF;
    if (h.in.fused_scan && gh_knn_scan_path(h)) return GH_SEARCH_FUSED;
    return gh_knn_scan_path(h) ? GH_SEARCH_SCAN : GH_SEARCH_BLOCK;   // gh_knn_local
}
// presetup_ids (api.hip) and the `gathered` branch of gh_launch_normalise (forces.hip)
bool presetup(const engine &h) {
    return h.in.rows == h.in.n && h.in.layout != GH_LAYOUT_GATHERED && gh_knn_scan_path(h) &&
           (h.in.fused_scan || gh_grid_path(h) || gh_ivf_path(h)) && h.in.S > 0 && h.in.k > 0 && !h.opt_no_presetup;
}
bool presetup_gathered(const engine &h) {
    return h.in.fused_scan && gh_knn_scan_path(h) && h.in.S > 0 && h.in.k > 0 && !h.opt_no_presetup;
}
// gh_launch_integrate (forces.hip): d_setup_rows exists (allocate_and_upload) and the finish is the single-rank one
bool stage_rows(const engine &h) { return h.thr_M1 > 0 && h.in.rows == h.in.n && h.in.layout == GH_LAYOUT_NONE; }
// launch_select (knn.hip) and gh_knn_finish_cdist (cdist.hip)
bool reduce(const engine &h, bool new0_ready) { return new0_ready && h.in.rows > 0 && h.in.LD <= 16 && h.in.S < 2048; }
// gh_get_scan_filter (api.hip)
int reported_filter(const engine &h) {
    return !gh_fused_uses_mfma(h) || h.in.D > 3 ? GH_FILTER_AUTO : h.qcells ? GH_FILTER_CELLS : GH_FILTER_MFMA;
}
// gh_create (api.hip): GRAPHEM_HIP_TAU_SEPARATE unset / 1 / 0
engine make(const gh_plan_input &in, const gh_plan_requests &rq) {
    engine h{};
    h.in = in;
    h.scan_filter = rq.scan_filter;
    h.coarse_mode = rq.coarse_mode;
    h.opt_no_presetup = rq.no_presetup;
    gh_choose_threshold_subset(h);
    h.tau_embedded_plan = rq.tau_place == GH_TAU_BY_SIZE ? in.n_vblocks <= 2048 : rq.tau_place == GH_TAU_EMBEDDED;
    gh_choose_scan_filter(h);
    return h;
}
}  // namespace old

static long cases = 0;

static void check_case(const gh_plan_input &in, const gh_plan_requests &rq) {
    ++cases;
    const old::engine h = old::make(in, rq);
    const gh_step_plan p = gh_make_step_plan(in, rq);
    const gh_search search = old::search(h);

    CHECK(p.search == search);
    CHECK(p.lists() == old::gh_knn_scan_path(h));
    CHECK((p.built == GH_SEARCH_GRID) == old::gh_grid_path(h));
    CHECK((p.built == GH_SEARCH_IVF) == old::gh_ivf_path(h));
    CHECK(p.built != GH_SEARCH_NONE && (search == GH_SEARCH_NONE || search == p.built));
    CHECK(p.thr_stride == h.thr_stride && p.thr_M1 == h.thr_M1);
    CHECK(p.cells_ok == old::gh_fused_cells_ok(h));
    CHECK(p.coarse_ok == old::gh_coarse_tau_ok(h));
    CHECK((p.prefilter == GH_PRE_CELLS) == h.qcells);
    CHECK((p.prefilter != GH_PRE_NONE) == old::gh_fused_uses_mfma(h));
    CHECK((p.prefilter == GH_PRE_WIDE_F16) == (old::gh_fused_uses_mfma(h) && in.D > 3));
    CHECK((p.prefilter == GH_PRE_SPLIT_F16 ? 0 : -1) == old::gh_fused_mfma_kb(h));   // operand rows the thresholds write
    const int reported = p.prefilter == GH_PRE_CELLS ? GH_FILTER_CELLS : p.prefilter == GH_PRE_SPLIT_F16 ? GH_FILTER_MFMA : GH_FILTER_AUTO;
    CHECK(reported == old::reported_filter(h));
    // the threshold form: what the old flags made the fused step do, a launch of their own for the unfused filtered scan
    const gh_tau_form tau = search == GH_SEARCH_FUSED ? (h.coarse_tau ? GH_TAUF_COARSE : h.tau_embedded ? GH_TAUF_EMBEDDED : GH_TAUF_LAUNCH)
                            : search == GH_SEARCH_SCAN ? GH_TAUF_LAUNCH : GH_TAUF_NONE;
    CHECK(p.tau == tau);
    CHECK(p.presetup == old::presetup(h));
    CHECK(p.presetup_gathered == old::presetup_gathered(h));
    CHECK(p.stage_rows == old::stage_rows(h));
    for (bool new0 : {false, true}) {
        gh_step_state s;
        s.new0_ready = new0;
        CHECK(gh_sums_ride_along(p, s) == old::reduce(h, new0));
    }

    // structural facts
    CHECK(p.tau != GH_TAUF_COARSE || p.prefilter == GH_PRE_CELLS);                                 // coarse implies cells
    CHECK(p.tau != GH_TAUF_EMBEDDED || p.prefilter != GH_PRE_CELLS);                               // embedded excludes cells
    CHECK((p.tau == GH_TAUF_NONE) == !(p.search == GH_SEARCH_FUSED || p.search == GH_SEARCH_SCAN));
    CHECK(p.prefilter != GH_PRE_CELLS || (in.D <= 3 && in.S <= GH_QC_SMAX));
    CHECK(!p.coarse_ok || p.cells_ok);
    CHECK((p.thr_M1 > 0) == (p.built == GH_SEARCH_FUSED || p.built == GH_SEARCH_SCAN));
}

// A whole-graph engine on a random 8-regular graph of n vertices, as bench.py creates it: 4 n edges, 256 queries, 10
// neighbours, one fused workgroup per 512 owned edges.
static gh_plan_input bench_engine(int64_t n, int D) {
    gh_plan_input in;
    in.n = in.rows = n;
    in.E = in.own_count = 4 * n;
    in.S = 256;
    in.D = D; in.LD = gh_ld(D);
    in.k = 10; in.K = 11; in.Ksel = 11;
    in.knn_method = GH_KNN_SCAN;
    in.fused_scan = true;
    in.n_vblocks = (int)((in.own_count + GH_FUSED_TILE - 1) / GH_FUSED_TILE);
    return in;
}

int main() {
    static_assert(GH_FUSED_TILE == 512 && GH_THR_TILE % GH_THR_GSIZE == 0, "the sizes the kernels were written for");
    for (int D : {1, 2, 3, 4, 6, 8, 16, 17})
    for (int64_t S : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)2047, (int64_t)2048, (int64_t)12288})
    for (int k : {1, 10, 11, 12, 30, 31, 32, 127, 128})
    for (int64_t own : {(int64_t)0, (int64_t)4095, (int64_t)4096, (int64_t)16383, (int64_t)16384, (int64_t)262144, (int64_t)4000000})
    for (int method : {GH_KNN_AUTO, GH_KNN_SCAN, GH_KNN_GRID, GH_KNN_IVF})
    for (bool cdist : {false, true})
    for (bool whole : {true, false})
    for (bool fused : {false, true})
    for (int vblocks : {1, 2048, 2049})
    if (fused || vblocks == 1)   // (an engine without the fused kernel has no workgroups of it)
    for (int layout : {(int)GH_LAYOUT_NONE, (int)GH_LAYOUT_GATHERED, (int)GH_LAYOUT_OVERLAP}) {
        gh_plan_input in;
        in.E = whole ? own : 2 * own;
        in.own_count = own;
        in.n = own / 4 + 1;
        in.rows = whole ? in.n : in.n / 2;
        in.S = S < in.E ? S : in.E;
        in.D = D; in.LD = gh_ld(D);
        in.k = k; in.K = k + 1; in.Ksel = in.K + (cdist ? 1 : 0);
        in.knn_method = method;
        in.cdist = cdist; in.cd_part = cdist && !whole;
        in.fused_scan = fused; in.n_vblocks = fused ? vblocks : 0;
        in.layout = layout;
        for (int filter : {GH_FILTER_AUTO, GH_FILTER_MFMA, GH_FILTER_CELLS})
        for (int coarse : {GH_COARSE_AUTO, GH_COARSE_OFF, GH_COARSE_ON})
        for (gh_tau_place place : {GH_TAU_BY_SIZE, GH_TAU_SEPARATE, GH_TAU_EMBEDDED})
        for (bool no_presetup : {false, true}) {
            gh_plan_requests rq;
            rq.scan_filter = filter; rq.coarse_mode = coarse; rq.tau_place = place; rq.no_presetup = no_presetup;
            check_case(in, rq);
        }
    }
    // k = 0 (no neighbours asked for) beside the S = 0 of the sweep
    {
        gh_plan_input in = bench_engine(1000000, 3);
        in.k = 0; in.K = in.Ksel = 1;
        check_case(in, gh_plan_requests{});
        CHECK(gh_make_step_plan(in, gh_plan_requests{}).search == GH_SEARCH_NONE);
    }

    // the benchmark's workloads with everything on its default
    const gh_plan_requests defaults;
    {   // rr1m: more than 2048 fused workgroups -> thresholds outside the launch's other workgroups -> cells, coarse
        const gh_step_plan p = gh_make_step_plan(bench_engine(1000000, 3), defaults);
        CHECK(p.search == GH_SEARCH_FUSED && p.prefilter == GH_PRE_CELLS && p.tau == GH_TAUF_COARSE);
        CHECK(p.presetup && p.stage_rows && p.coarse_ok);
    }
    {   // rr100k: one round of workgroups -> thresholds inside the launch -> the split-f16 filter stays
        const gh_step_plan p = gh_make_step_plan(bench_engine(100000, 3), defaults);
        CHECK(p.search == GH_SEARCH_FUSED && p.prefilter == GH_PRE_SPLIT_F16 && p.tau == GH_TAUF_EMBEDDED);
    }
    {   // rr1m_d6: no cell table beyond three components -> the wide filter, thresholds in a launch of their own
        const gh_step_plan p = gh_make_step_plan(bench_engine(1000000, 6), defaults);
        CHECK(p.search == GH_SEARCH_FUSED && p.prefilter == GH_PRE_WIDE_F16 && p.tau == GH_TAUF_LAUNCH);
    }

    if (failures) { std::fprintf(stderr, "%ld check(s) failed over %ld cases\n", failures, cases); return 1; }
    std::printf("step_plan_host_check: ok (%ld cases)\n", cases);
    return 0;
}
