// What a row-partitioned engine exchanges to finish a step, and where it lies: one value, made by one pure function of the
// engine's sizes and the caller's (world, rank, chunk).  Plain C++17, no HIP: it compiles with a host compiler alone
// (tools/exchange_layout_host_check.cpp sweeps it against the expressions it replaced).  DESIGN.md section 6 has the table.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>

#include "../../include/graphem_hip.h"   // gh_status

// How a partitioned engine finishes a step (include/graphem_hip.h): set by gh_gather_layout (form B), gh_rank_layout
// (form C), gh_overlap_layout (form D).
enum { GH_LAYOUT_NONE = 0, GH_LAYOUT_GATHERED, GH_LAYOUT_RANK, GH_LAYOUT_OVERLAP };

// Row pairs of corrections behind the (2, LD) column statistics: one per stats_fix workgroup.
inline int gh_fix_blocks(int LD) { return LD <= 16 ? 2 * LD : 0; }
// Statistics rows of a rank: sum, sum of squares, then the correction row pairs.
inline int gh_stats_rows(int LD) { return 2 + 2 * gh_fix_blocks(LD); }

// A rank's buffers are (world, ...) arrays of equal blocks in rank order, so that an all-gather fills them in place:
//   rows     form B: the slots, [chunk rows of LD floats | statistics rows], slot_bytes each (a multiple of 16);
//            form D: (world, chunk, LD) the un-normalised rows new0 = pos + Fs; form C: none (the rows are in d_pos)
//   packed   forms C and D with D < LD and world > 1: (world, chunk, D) the rows without their pad columns -- what travels
//            (12 instead of 16 bytes per row at 3 components)
//   late     form D: (world, late_doubles) per rank its statistics rows, then its PATCH LIST: two int32 counters used by
//            alternate iterations (16 bytes reserved) and patch_cap records (row as int32 bits, LD floats) -- the own rows
//            the intersection phase touched, as finished by their owner, pos + (Fs + Fi)
// Offsets are in elements of the buffer they index (floats of rows / packed, doubles of late -- form B: of rows).
struct gh_exchange_layout {
    int form = GH_LAYOUT_NONE;
    int world = 0, rank = 0;
    int64_t chunk = 0;            // rows per rank block
    int D = 0, LD = 0;
    int64_t slot_bytes = 0;       // form B: bytes of a slot (0 otherwise)
    int row_floats = 0;           // floats per travelling row: D where a packed buffer exists, else LD
    int64_t block_floats = 0;     // floats between two ranks' rows as the all-rows finish reads them (forms B, D; 0: form C)
    int64_t stats_doubles = 0;    // doubles of a rank's statistics rows: gh_stats_rows(LD) * LD
    int64_t late_doubles = 0;     // doubles between two ranks' statistics where they are gathered: the slot (B), the
                                  // statistics rows (C, in the caller's buffer), statistics + patch list (D)
    int64_t patch_cap = 0;        // form D: patch records per rank, min(4 S k, chunk), at least 1
    bool packed_default = false;  // form C: the packed block exchange is on unless the caller says otherwise (from 2 M
                                  // vertices on, where the saved quarter of the all-gather outweighs the expansion kernel
                                  // -- 30 us at 4 M vertices, 14 at 1 M)
    // elements each buffer takes (0: the form has none)
    int64_t rows_floats = 0, packed_floats = 0, late_all_doubles = 0;
    // where things lie
    int64_t first_stats = 0;      // doubles from the start of the statistics' buffer to rank 0's statistics rows
    int64_t own_rows = 0;         // floats to the own block of rows
    int64_t own_packed = 0;       // floats to the own block of packed (or of an unpadded (world, chunk, D) array)
    int64_t own_pos = 0;          // floats to the own block of the position array (form C, unpacked)
    int64_t own_stats = 0;        // doubles to the own statistics rows = first_stats + rank * late_doubles
    int64_t patch_counters = 0;   // doubles from a rank's statistics rows to its two int32 patch counters ...
    int64_t patch_records = 0;    // ... and to its first patch record

    bool packed_rows() const { return packed_floats > 0; }
    // bytes a rank sends in an exchange: its slot, its late block, its block of rows (packed or padded)
    size_t late_bytes() const { return sizeof(double) * (size_t)late_doubles; }
    size_t rows_block_bytes(bool packed) const { return sizeof(float) * (size_t)chunk * (size_t)(packed ? D : LD); }
};

// The engine's sizes a layout depends on.
struct gh_layout_input {
    int64_t n = 0, pos_rows = 0;   // vertices, rows allocated in the position array
    int D = 0, LD = 0;
    int64_t S = 0;
    int k = 0;
    int64_t row_lo = 0, row_hi = 0;   // the engine's row partition
};

// The layout of `form` for world blocks of chunk rows, block `rank` the engine's row partition (form C: the blocks within
// the position array); current: the form the engine has (a layout is set once).  A refusal leaves *out alone.
inline gh_status gh_make_exchange_layout(const gh_layout_input &in, int current, int form, int32_t world, int32_t rank, int64_t chunk,
                                         gh_exchange_layout *out, std::string *err) {
    const char *what = form == GH_LAYOUT_GATHERED ? "gather layout" : form == GH_LAYOUT_RANK ? "rank layout" : "overlap layout";
    const bool within_pos = form == GH_LAYOUT_RANK;
    if (world < 1 || rank < 0 || rank >= world || chunk < 1 || chunk * world < in.n || (within_pos && chunk * world > in.pos_rows) ||
        in.row_lo != std::min<int64_t>(in.n, rank * chunk) || in.row_hi != std::min<int64_t>(in.n, (rank + 1) * chunk)) {
        *err = std::string(what) + " does not match the engine's row partition";
        return GH_ERR_INVALID;
    }
    if (current != GH_LAYOUT_NONE) { *err = "rank / gather layout already set"; return GH_ERR_INVALID; }
    if (form == GH_LAYOUT_OVERLAP && in.LD > 16) {
        *err = "gh_overlap_layout: up to 16 components (use gh_rank_layout / gh_gather_layout beyond)";
        return GH_ERR_INVALID;
    }
    gh_exchange_layout l;
    l.form = form; l.world = world; l.rank = rank; l.chunk = chunk; l.D = in.D; l.LD = in.LD;
    l.stats_doubles = (int64_t)gh_stats_rows(in.LD) * in.LD;
    const int64_t block_rows_floats = chunk * in.LD;
    // fewer components than the row stride (3 of 4, 5..7 of 8, 9..15 of 16): the blocks travel unpadded
    if (form != GH_LAYOUT_GATHERED && in.D < in.LD && world > 1) l.packed_floats = (int64_t)world * chunk * in.D;
    l.row_floats = l.packed_rows() ? in.D : in.LD;
    l.own_packed = (int64_t)rank * chunk * in.D;
    l.own_pos = (int64_t)rank * block_rows_floats;
    if (form == GH_LAYOUT_GATHERED) {
        l.slot_bytes = (block_rows_floats * (int64_t)sizeof(float) + l.stats_doubles * (int64_t)sizeof(double) + 15) / 16 * 16;
        l.rows_floats = l.slot_bytes * world / (int64_t)sizeof(float);
        l.block_floats = l.slot_bytes / (int64_t)sizeof(float);
        l.late_doubles = l.slot_bytes / (int64_t)sizeof(double);
        l.first_stats = block_rows_floats / 2;   // (the row stride is a multiple of 4 floats)
        l.own_rows = (int64_t)rank * l.block_floats;
    } else if (form == GH_LAYOUT_RANK) {
        l.late_doubles = l.stats_doubles;
        l.packed_default = l.packed_rows() && in.n >= ((int64_t)1 << 21);
    } else {
        // a rank's block of the late all-gather: statistics rows, 16 bytes for the patch counters, the patch records
        l.patch_cap = std::max<int64_t>(1, std::min<int64_t>(4 * in.S * in.k, chunk));
        l.late_doubles = l.stats_doubles + 2 + (l.patch_cap * (1 + in.LD) * 4 + 7) / 8;
        l.late_doubles = (l.late_doubles + 1) / 2 * 2;   // 16-byte multiples
        l.rows_floats = (int64_t)world * block_rows_floats;
        l.late_all_doubles = (int64_t)world * l.late_doubles;
        l.block_floats = chunk * l.row_floats;
        l.own_rows = (int64_t)rank * block_rows_floats;
        l.patch_counters = l.stats_doubles;
        l.patch_records = l.stats_doubles + 2;
    }
    l.own_stats = l.first_stats + (int64_t)rank * l.late_doubles;
    *out = l;
    return GH_OK;
}
