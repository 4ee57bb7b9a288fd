// The exchange layout (graphem-rapids_amd/csrc/exchange_layout.h) as a stand-alone host program:
//
//     g++ -std=c++17 -O2 -Wall -Werror tools/exchange_layout_host_check.cpp -o exchange_layout_host_check && ./exchange_layout_host_check
//
// The oracle below is a frozen restatement of what the layout replaced: check_layout and the three setters of api.hip, and
// the expressions gh_patch_count, gh_launch_normalise, gh_launch_pack_rows, gh_launch_patch_rows (engine.h, forces.hip),
// comm_common and gh_run_partitioned (comm.hip) derived from the engine members those setters wrote (names kept), with
// byte addresses standing in for the device pointers.  The sweep asserts that every field of the value is what they imply.
// Exit status 0: every check held (tests/test_step_plan_host.py).
#include <cstdio>
#include <initializer_list>

#include "../graphem-rapids_amd/csrc/dispatch.h"    // gh_ld
#include "../graphem-rapids_amd/csrc/exchange_layout.h"

static long failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { if (++failures <= 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); } } while (0)

// ---- the oracle ------------------------------------------------------------------------------------------------------
namespace old {
int fix_blocks(int LD) { return LD <= 16 ? 2 * LD : 0; }
struct engine {
    int64_t n, pos_rows, S, row_lo, row_hi;
    int D, LD, k;
    // what the setters wrote; a buffer is its element count (0: not allocated), a view is a byte offset into its buffer
    int64_t d_gbuf = 0, g_slot = 0, g_chunk = 0;
    int g_world = 0, g_rank = 0;
    int layout = GH_LAYOUT_NONE;
    int64_t d_rows_packed = 0, d_rows_all = 0, d_rows_pk = 0, d_stats_all = 0, stats_block = 0, patch_cap = 0;
    bool packed_exchange = false;
    int64_t d_new = -1, d_stats = -1;   // bytes into d_gbuf (form B) / d_rows_all and d_stats_all (form D)
    std::string err;
};
gh_status check_layout(engine *h, const char *what, int32_t world, int32_t rank, int64_t chunk, bool within_pos = false) {
    if (world < 1 || rank < 0 || rank >= world || chunk < 1 || chunk * world < h->n || (within_pos && chunk * world > h->pos_rows) ||
        h->row_lo != std::min<int64_t>(h->n, rank * chunk) || h->row_hi != std::min<int64_t>(h->n, (rank + 1) * chunk)) {
        h->err = std::string(what) + " does not match the engine's row partition";
        return GH_ERR_INVALID;
    }
    if (h->layout != GH_LAYOUT_NONE) { h->err = "rank / gather layout already set"; return GH_ERR_INVALID; }
    return GH_OK;
}
gh_status gh_gather_layout(engine *h, int32_t world, int32_t rank, int64_t chunk) {
    if (gh_status st = check_layout(h, "gather layout", world, rank, chunk)) return st;
    const int64_t stats_bytes = (int64_t)sizeof(double) * (2 + 2 * fix_blocks(h->LD)) * h->LD;
    const int64_t slot = (chunk * h->LD * (int64_t)sizeof(float) + stats_bytes + 15) / 16 * 16;
    h->d_gbuf = slot * world;
    h->d_new = rank * slot;
    h->d_stats = rank * slot + chunk * h->LD * (int64_t)sizeof(float);
    h->g_slot = slot; h->g_chunk = chunk; h->g_world = world; h->g_rank = rank;
    h->layout = GH_LAYOUT_GATHERED;
    return GH_OK;
}
gh_status gh_rank_layout(engine *h, int32_t world, int32_t rank, int64_t chunk) {
    if (gh_status st = check_layout(h, "rank layout", world, rank, chunk, true)) return st;
    if (h->D < h->LD && world > 1) {
        h->d_rows_packed = (int64_t)world * chunk * h->D;
        h->packed_exchange = h->n >= ((int64_t)1 << 21);
    }
    h->g_chunk = chunk; h->g_world = world; h->g_rank = rank;
    h->layout = GH_LAYOUT_RANK;
    return GH_OK;
}
gh_status gh_overlap_layout(engine *h, int32_t world, int32_t rank, int64_t chunk) {
    if (gh_status st = check_layout(h, "overlap layout", world, rank, chunk)) return st;
    if (h->LD > 16) { h->err = "gh_overlap_layout: up to 16 components (use gh_rank_layout / gh_gather_layout beyond)"; return GH_ERR_INVALID; }
    const int64_t R = 2 + 2 * fix_blocks(h->LD);
    h->patch_cap = std::max<int64_t>(1, std::min<int64_t>(4 * h->S * h->k, chunk));
    h->stats_block = (int64_t)(R * h->LD) + 2 + ((int64_t)h->patch_cap * (1 + h->LD) * 4 + 7) / 8;
    h->stats_block = (h->stats_block + 1) / 2 * 2;
    h->d_rows_all = (int64_t)world * chunk * h->LD;
    h->d_stats_all = (int64_t)world * h->stats_block;
    if (h->D < h->LD && world > 1) h->d_rows_pk = (int64_t)world * chunk * h->D;
    h->d_new = (int64_t)sizeof(float) * rank * chunk * h->LD;
    h->d_stats = (int64_t)sizeof(double) * rank * h->stats_block;
    h->g_chunk = chunk; h->g_world = world; h->g_rank = rank;
    h->layout = GH_LAYOUT_OVERLAP;
    return GH_OK;
}
}  // namespace old

static long cases = 0, accepted = 0;

static void check_case(const gh_layout_input &in, int current, int form, int32_t world, int32_t rank, int64_t chunk) {
    ++cases;
    old::engine h{};
    h.n = in.n; h.pos_rows = in.pos_rows; h.S = in.S; h.row_lo = in.row_lo; h.row_hi = in.row_hi;
    h.D = in.D; h.LD = in.LD; h.k = in.k;
    h.layout = current;
    const gh_status want = form == GH_LAYOUT_GATHERED ? old::gh_gather_layout(&h, world, rank, chunk)
                           : form == GH_LAYOUT_RANK   ? old::gh_rank_layout(&h, world, rank, chunk)
                                                      : old::gh_overlap_layout(&h, world, rank, chunk);
    gh_exchange_layout l;
    std::string err;
    const gh_status got = gh_make_exchange_layout(in, current, form, world, rank, chunk, &l, &err);
    CHECK(got == want && err == h.err);
    if (want != GH_OK) { CHECK(l.form == GH_LAYOUT_NONE); return; }   // a refusal leaves the value alone
    ++accepted;
    const int64_t R = 2 + 2 * old::fix_blocks(h.LD), F = sizeof(float), Dbl = sizeof(double);
    CHECK(gh_stats_rows(h.LD) == R && l.stats_doubles == R * h.LD);
    CHECK(l.form == h.layout && l.world == h.g_world && l.rank == h.g_rank && l.chunk == h.g_chunk && l.D == h.D && l.LD == h.LD);
    // the buffers
    CHECK(l.slot_bytes == h.g_slot && l.patch_cap == h.patch_cap);
    CHECK(l.rows_floats * F == (form == GH_LAYOUT_GATHERED ? h.d_gbuf : h.d_rows_all * F));
    CHECK(l.packed_floats == (form == GH_LAYOUT_RANK ? h.d_rows_packed : h.d_rows_pk));
    CHECK(l.late_all_doubles == h.d_stats_all);
    CHECK(l.packed_default == h.packed_exchange);
    // the views d_new and d_stats (forms B, D; form C leaves them where they are)
    if (form != GH_LAYOUT_RANK) CHECK(l.own_rows * F == h.d_new && l.own_stats * Dbl == h.d_stats);
    // gh_rows_all_row_floats, gh_stats_all_block_doubles
    if (form == GH_LAYOUT_OVERLAP) CHECK(l.row_floats == (h.d_rows_pk ? h.D : h.LD) && l.late_doubles == h.stats_block);
    // gh_patch_count: d_stats + R * LD doubles; gh_patch_records: four int32 further; patch_rows_kernel's stat_doubles
    if (form == GH_LAYOUT_OVERLAP) CHECK(l.patch_counters == R * h.LD && l.patch_records * Dbl == l.patch_counters * Dbl + 4 * 4);
    // gh_launch_normalise: form C's statistics; forms B / D: RS, block, stats, stats_block (and the packed own block of form C)
    if (form == GH_LAYOUT_RANK) CHECK(l.late_doubles == R * h.LD);
    else {
        const bool overlap = form == GH_LAYOUT_OVERLAP;
        const int RS = overlap && h.d_rows_pk ? h.D : h.LD;
        CHECK(l.row_floats == RS);
        CHECK(l.block_floats == (overlap ? h.g_chunk * RS : h.g_slot / F));
        CHECK(l.first_stats * Dbl == (overlap ? 0 : h.g_chunk * h.LD * F));
        CHECK(l.late_doubles == (overlap ? h.stats_block : h.g_slot / Dbl));
        CHECK(l.own_stats == l.first_stats + l.rank * l.late_doubles);
    }
    CHECK(l.own_packed == (int64_t)h.g_rank * h.g_chunk * h.D);   // forces.hip: normalise (form C), gh_launch_pack_rows (form D)
    // gh_run_partitioned: the bytes a rank sends, and where its block lies
    if (form == GH_LAYOUT_OVERLAP) {
        CHECK((int64_t)l.rows_block_bytes(l.packed_rows()) == F * h.g_chunk * (h.d_rows_pk ? h.D : h.LD));
        CHECK((int64_t)l.late_bytes() == Dbl * h.stats_block);
    } else if (form == GH_LAYOUT_RANK) {
        CHECK((int64_t)l.late_bytes() == Dbl * R * h.LD);
        CHECK((int64_t)l.rows_block_bytes(true) == F * h.g_chunk * h.D && (int64_t)l.rows_block_bytes(false) == F * h.g_chunk * h.LD);
        CHECK(l.own_pos * F == h.g_rank * (int64_t)l.rows_block_bytes(false));
    } else {
        CHECK(l.own_rows * F == h.g_rank * h.g_slot);
    }
    // structural facts the callers rely on: 16-byte blocks, views inside their buffers
    CHECK(l.slot_bytes % 16 == 0 && l.late_bytes() % (form == GH_LAYOUT_RANK ? 8 : 16) == 0);
    if (form != GH_LAYOUT_RANK) {
        CHECK(l.own_rows + l.chunk * l.LD <= l.rows_floats);
        const int64_t stats_buffer = form == GH_LAYOUT_GATHERED ? l.rows_floats / 2 : l.late_all_doubles;
        CHECK(l.own_stats + l.stats_doubles <= stats_buffer);
        if (form == GH_LAYOUT_OVERLAP) CHECK(l.patch_records * Dbl + l.patch_cap * (1 + l.LD) * F <= l.late_doubles * Dbl);
    }
    if (l.packed_rows()) CHECK(l.own_packed + l.chunk * l.D <= l.packed_floats);
}

int main() {
    for (int64_t n : {(int64_t)1, (int64_t)3, (int64_t)9, (int64_t)1000, (int64_t)20001, ((int64_t)1 << 21) - 1, (int64_t)1 << 21})
    for (int world = 1; world <= 8; ++world)
    for (int rank = 0; rank < world; ++rank)
    for (int LD : {4, 8, 16, 20})
    for (int D : {1, LD - 1, LD})
    if (gh_ld(D) == LD)
    for (int64_t Sk : {(int64_t)0, (int64_t)1, (int64_t)100, (int64_t)2560})
    for (int form : {(int)GH_LAYOUT_GATHERED, (int)GH_LAYOUT_RANK, (int)GH_LAYOUT_OVERLAP}) {
        const int64_t chunk = (n + world - 1) / world;   // distributed.partition_rows: n < world leaves the last ranks empty
        gh_layout_input in;
        in.n = n; in.pos_rows = n + 1024;
        in.D = D; in.LD = LD;
        in.S = Sk ? Sk / (Sk >= 10 ? 10 : 1) : 0; in.k = Sk >= 10 ? 10 : Sk ? 1 : 0;
        in.row_lo = std::min<int64_t>(n, rank * chunk);
        in.row_hi = std::min<int64_t>(n, in.row_lo + chunk);
        check_case(in, GH_LAYOUT_NONE, form, world, rank, chunk);
        // refusals: a second layout, another rank's block, a chunk too small, blocks beyond the position array (form C)
        for (int current : {(int)GH_LAYOUT_GATHERED, (int)GH_LAYOUT_RANK, (int)GH_LAYOUT_OVERLAP}) check_case(in, current, form, world, rank, chunk);
        check_case(in, GH_LAYOUT_NONE, form, world, rank + 1, chunk);
        check_case(in, GH_LAYOUT_NONE, form, world, -1, chunk);
        check_case(in, GH_LAYOUT_NONE, form, 0, rank, chunk);
        check_case(in, GH_LAYOUT_NONE, form, world, rank, chunk - 1);
        check_case(in, GH_LAYOUT_NONE, form, world, rank, chunk + 1);
        if (rank == 0 && world == 1) check_case(in, GH_LAYOUT_NONE, form, world, rank, n + 1025);
    }
    // the default exchange of the benchmark: 1 M vertices, three components, 256 queries of 10 neighbours, eight ranks
    {
        gh_layout_input in;
        in.n = 1000000; in.pos_rows = in.n + 1024; in.D = 3; in.LD = 4; in.S = 256; in.k = 10;
        in.row_lo = 125000; in.row_hi = 250000;
        gh_exchange_layout l;
        std::string err;
        CHECK(gh_make_exchange_layout(in, GH_LAYOUT_NONE, GH_LAYOUT_OVERLAP, 8, 1, 125000, &l, &err) == GH_OK);
        CHECK(l.row_floats == 3 && l.patch_cap == 10240 && l.rows_block_bytes(true) == 1500000 && l.late_doubles == 18 * 4 + 2 + 25600);
    }
    if (failures) { std::fprintf(stderr, "%ld check(s) failed over %ld cases\n", failures, cases); return 1; }
    std::printf("exchange_layout_host_check: ok (%ld cases, %ld accepted)\n", cases, accepted);
    return 0;
}
