// Edge-list ingestion (include/graphem_hip.h "edge-list ingestion"): the text of a SNAP / .edges / .mtx file to
// (vertices, edges), behind gh_ingest_*.  The rule for one line is ingest_parse_line (ingest_core.h), compiled for both
// sides; the host path (device_id < 0) is ingest_core.h's, so both paths give the same arrays.
//
// Per chunk of text (cut by the host after a whole terminator):
//   ing_starts_kernel    a lane loads 16 consecutive bytes with one dwordx4 and builds the mask of line starts among them
//                        (the byte before is LF, or is CR and this byte is not LF; the chunk's first byte always); pass 0
//                        stores the popcount, an exclusive scan (hipCUB) follows, pass 1 stores the offsets in order
//   ing_parse_kernel     a lane per line: comment test, two fields, sign, digits, overflow; (a, b, is-row); a bad line
//                        takes the minimum of its file offset into one word -- the only atomic whose value is ever read,
//                        and a minimum does not depend on order.  Every read is inside [line start, next line start).
//   ing_compact_kernel   after a scan of the is-row flags: the rows, in file order, behind those of earlier chunks
// After the last chunk:
//   labels as sign-flipped 64-bit keys -> radix sort -> unique: the label table; every label's dense id by binary search;
//   undirected: keys (lo << 32) | hi with self-loops as an all-ones sentinel -> sort -> unique; for vertices_from =
//   'edges' the table is re-ranked to the labels that survive by flags and a scan.
// A line is never split over lanes, so a 10 000-byte comment or 5 000 blanks between two fields are one lane's loop.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host_util.h"
#include "ingest_core.h"

#define ING_BLOCK 256
#define ING_DEFAULT_BUDGET (4ll << 30)
#define ING_MAX_CHUNK (1ll << 30)
#define ING_MAX_ROWS (1ll << 30)
#define ING_NO_ERROR 0xFFFFFFFFFFFFFFFFull
#define ING_SIGN 0x8000000000000000ull

namespace {

// Line starts among bytes [16 w, 16 w + 16) of `text` (16-byte aligned, `cap` bytes allocated), limited to [lo, hi).
__device__ __forceinline__ uint32_t ing_start_mask(const uint8_t *__restrict__ text, int64_t w, int64_t lo, int64_t hi, int64_t cap) {
    const int64_t base = 16 * w;
    uint32_t q[4] = {0, 0, 0, 0};
    if (base + 16 <= cap) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + base);
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    } else {
        for (int k = 0; k < 16; ++k)
            if (base + k < cap) q[k >> 2] |= (uint32_t)text[base + k] << (8 * (k & 3));
    }
    uint32_t prev = base > lo ? text[base - 1] : '\n';
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = (q[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        const int64_t i = base + k;
        const bool start = prev == '\n' || (prev == '\r' && c != '\n') || i == lo;
        if (start && i >= lo && i < hi) mask |= 1u << k;
        prev = c;
    }
    return mask;
}

// pass 0: counts[g] = line starts of lane g's 16 bytes.  pass 1: starts[offs[g] ..] = their offsets from lo, ascending.
__global__ __launch_bounds__(ING_BLOCK) void ing_starts_kernel(const uint8_t *__restrict__ text, int64_t lo, int64_t hi, int64_t cap,
                                                               int64_t n_words, int pass, int32_t *__restrict__ counts,
                                                               const int32_t *__restrict__ offs, uint32_t *__restrict__ starts) {
    const int64_t g = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (g >= n_words) return;
    const int64_t w = lo / 16 + g;
    uint32_t mask = ing_start_mask(text, w, lo, hi, cap);
    if (pass == 0) { counts[g] = __popc(mask); return; }
    int64_t out = offs[g];
    while (mask) {
        const int k = __ffs(mask) - 1;
        mask &= mask - 1;
        starts[out++] = (uint32_t)(16 * w + k - lo);
    }
}

__global__ __launch_bounds__(ING_BLOCK) void ing_parse_kernel(const uint8_t *__restrict__ chunk, int64_t len, int64_t file_off, int64_t n_lines,
                                                              const uint32_t *__restrict__ starts, int comment, int dec,
                                                              int64_t *__restrict__ ab, int32_t *__restrict__ is_row,
                                                              unsigned long long *__restrict__ first_bad) {
    const int64_t l = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (l >= n_lines) return;
    const int64_t s = starts[l], e = l + 1 < n_lines ? (int64_t)starts[l + 1] : len;
    int64_t a = 0, b = 0, at, ln;
    const int k = ingest_parse_line(chunk + s, e - s, comment, dec, &a, &b, &at, &ln);
    ab[2 * l] = a;
    ab[2 * l + 1] = b;
    is_row[l] = k == INGEST_ROW;
    if (k >= INGEST_BAD_INT) atomicMin(first_bad, (unsigned long long)(file_off + s));
}

__global__ __launch_bounds__(ING_BLOCK) void ing_compact_kernel(int64_t n_lines, const int64_t *__restrict__ ab, const int32_t *__restrict__ is_row,
                                                                const int32_t *__restrict__ pos, int64_t *__restrict__ rows) {
    const int64_t l = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (l >= n_lines || !is_row[l]) return;
    rows[2 * (int64_t)pos[l]] = ab[2 * l];
    rows[2 * (int64_t)pos[l] + 1] = ab[2 * l + 1];
}

// int64 labels <-> keys whose unsigned order is the labels' signed order
__global__ __launch_bounds__(ING_BLOCK) void ing_flip_kernel(int64_t count, const uint64_t *__restrict__ in, uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (i < count) out[i] = in[i] ^ ING_SIGN;
}

__device__ __forceinline__ int64_t ing_lower_bound(const uint64_t *__restrict__ table, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (table[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// keys[r] = (lo id << 32) | hi id of row r, all ones for a self-loop.  Every label is in the table.
__global__ __launch_bounds__(ING_BLOCK) void ing_keys_kernel(int64_t R, const uint64_t *__restrict__ rows, const uint64_t *__restrict__ table,
                                                             int64_t n_table, uint64_t *__restrict__ keys) {
    const int64_t r = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (r >= R) return;
    const uint64_t u = (uint64_t)ing_lower_bound(table, n_table, rows[2 * r] ^ ING_SIGN);
    const uint64_t v = (uint64_t)ing_lower_bound(table, n_table, rows[2 * r + 1] ^ ING_SIGN);
    keys[r] = u == v ? ING_NO_ERROR : ((u < v ? u : v) << 32) | (u < v ? v : u);
}

// used[id] = 1 for both ends of every key: all stores write the same value
__global__ __launch_bounds__(ING_BLOCK) void ing_mark_kernel(int64_t E, const uint64_t *__restrict__ keys, int32_t *__restrict__ used) {
    const int64_t e = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (e >= E) return;
    used[keys[e] >> 32] = 1;
    used[keys[e] & 0xFFFFFFFFull] = 1;
}

// vertices[rank] = the label of table entry i, for the entries in use (used == NULL: all, rank = i)
__global__ __launch_bounds__(ING_BLOCK) void ing_vertices_kernel(int64_t n_table, const uint64_t *__restrict__ table, const int32_t *__restrict__ used,
                                                                 const int32_t *__restrict__ rank, int64_t *__restrict__ vertices) {
    const int64_t i = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (i >= n_table) return;
    if (!used) vertices[i] = (int64_t)(table[i] ^ ING_SIGN);
    else if (used[i]) vertices[rank[i]] = (int64_t)(table[i] ^ ING_SIGN);
}

__global__ __launch_bounds__(ING_BLOCK) void ing_ids_kernel(int64_t E, const uint64_t *__restrict__ keys, const int32_t *__restrict__ rank,
                                                            int32_t *__restrict__ ids) {
    const int64_t e = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int32_t u = (int32_t)(keys[e] >> 32), v = (int32_t)(keys[e] & 0xFFFFFFFFull);
    ids[2 * e] = rank ? rank[u] : u;
    ids[2 * e + 1] = rank ? rank[v] : v;
}

// out[i] for the 2 E endpoints: ids given -> the id or its label; else rows' labels -> their rank in vertices
__global__ __launch_bounds__(ING_BLOCK) void ing_edges_out_kernel(int64_t count, const int32_t *__restrict__ ids, const int64_t *__restrict__ rows,
                                                                  const int64_t *__restrict__ vertices, int64_t n_vertices, int relabel,
                                                                  int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * ING_BLOCK + threadIdx.x;
    if (i >= count) return;
    if (ids) { out[i] = relabel ? (int64_t)ids[i] : vertices[ids[i]]; return; }
    const int64_t x = rows[i];
    int64_t lo = 0, hi = n_vertices;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (vertices[mid] < x) lo = mid + 1; else hi = mid;
    }
    out[i] = lo;
}

unsigned ing_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + ING_BLOCK - 1) / ING_BLOCK); }

}  // namespace

struct gh_ingest : gh_host {            // device < 0: host path
    int64_t chunks = 0;
    bool parsed = false, directed = false;
    ingest_result host;                 // the host path's result
    int64_t R = 0, E = 0, n_vertices = 0;
    gh_dev<int64_t> d_rows;             // (R, 2) labels in file order; kept for a directed result
    int64_t rows_cap = 0;
    gh_dev<int64_t> d_vertices;
    gh_dev<int32_t> d_ids;              // (E, 2) ranks in d_vertices, undirected
    gh_dev<uint8_t> d_text;             // the chunk
    int64_t text_cap = 0;
    uint8_t *pinned = nullptr;
    int64_t pinned_cap = 0;
    gh_dev<void> d_tmp;                 // hipCUB's work space
    size_t tmp_cap = 0;
};

static thread_local std::string g_ingest_error;

namespace {

gh_status ing_invalid(gh_ingest *h, const std::string &msg) {
    h->err = msg;
    return GH_ERR_INVALID;
}

gh_status ing_nomem(gh_ingest *h, int64_t bytes, const char *what) {
    h->err = "hipMalloc failed for " + std::to_string(bytes) + " bytes of " + what;
    return GH_ERR_NOMEM;
}

gh_status ing_tmp(gh_ingest *h, size_t bytes) {
    if (bytes <= h->tmp_cap && h->d_tmp.p) return GH_OK;
    if (!h->d_tmp.alloc(bytes)) { h->tmp_cap = 0; return ing_nomem(h, (int64_t)bytes, "work space"); }
    h->tmp_cap = bytes;
    return GH_OK;
}

gh_status ing_scan(gh_ingest *h, const int32_t *in, int32_t *out, int64_t count) {
    size_t temp = 0;
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, in, out, (int)count, h->stream));
    GH_TRY_ST(ing_tmp(h, temp));
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(h->d_tmp.p, temp, in, out, (int)count, h->stream));
    return GH_OK;
}

// *total = out[count - 1] + in[count - 1] of a scan; count >= 1.  Synchronises.
gh_status ing_scan_total(gh_ingest *h, const int32_t *in, const int32_t *out, int64_t count, int64_t *total) {
    int32_t a = 0, b = 0;
    GH_HIP(hipMemcpyAsync(&a, in + count - 1, 4, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(&b, out + count - 1, 4, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    *total = (int64_t)a + b;
    return GH_OK;
}

// Sorts `count` keys of a <-> b and leaves the distinct ones, ascending, in *uniq (one of the two); *n_uniq = how many.
gh_status ing_sort_unique(gh_ingest *h, uint64_t *a, uint64_t *b, int64_t count, int32_t *d_num, uint64_t **uniq, int64_t *n_uniq) {
    hipcub::DoubleBuffer<uint64_t> db(a, b);
    size_t temp = 0;
    GH_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, temp, db, (int)count, 0, 64, h->stream));
    GH_TRY_ST(ing_tmp(h, temp));
    GH_HIP(hipcub::DeviceRadixSort::SortKeys(h->d_tmp.p, temp, db, (int)count, 0, 64, h->stream));
    uint64_t *sorted = db.Current(), *other = sorted == a ? b : a;
    GH_HIP(hipcub::DeviceSelect::Unique(nullptr, temp, sorted, other, d_num, (int)count, h->stream));
    GH_TRY_ST(ing_tmp(h, temp));
    GH_HIP(hipcub::DeviceSelect::Unique(h->d_tmp.p, temp, sorted, other, d_num, (int)count, h->stream));
    int32_t num = 0;
    GH_HIP(hipMemcpyAsync(&num, d_num, 4, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    *uniq = other;
    *n_uniq = num;
    return GH_OK;
}

// Room for `need` rows in d_rows; the rows already there are kept.
gh_status ing_rows_room(gh_ingest *h, int64_t have, int64_t need) {
    if (need <= h->rows_cap) return GH_OK;
    const int64_t cap = std::max<int64_t>(need, 2 * h->rows_cap);
    gh_dev<int64_t> grown;
    if (!grown.alloc(16 * (size_t)cap)) return ing_nomem(h, 16 * cap, "rows");
    if (have) GH_HIP(hipMemcpyAsync(grown.p, h->d_rows.p, 16 * (size_t)have, hipMemcpyDeviceToDevice, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    h->d_rows = std::move(grown);
    h->rows_cap = cap;
    return GH_OK;
}

int64_t ing_chunk_bytes(const gh_ingest *h) {
    return std::max<int64_t>(16, std::min<int64_t>(ING_MAX_CHUNK, h->budget / GH_INGEST_BUDGET_PER_BYTE));
}

// The rows of text[off, end) behind the R rows already in d_rows.  *bad = the file offset of the first bad line, if any.
gh_status ing_chunk(gh_ingest *h, const uint8_t *bytes, const uint8_t *d_bytes, int64_t nbytes, int64_t off, int64_t end, int format,
                    gh_dev<unsigned long long> &d_bad, uint64_t *bad) {
    const int64_t len = end - off;
    const uint8_t *text;
    int64_t lo, cap;
    if (d_bytes) {
        text = d_bytes; lo = off; cap = nbytes;
    } else {
        const int64_t padded = (len + 15) / 16 * 16;
        if (padded > h->text_cap) {
            if (!h->d_text.alloc((size_t)padded)) { h->text_cap = 0; return ing_nomem(h, padded, "text"); }
            h->text_cap = padded;
        }
        if (padded > h->pinned_cap) {
            if (h->pinned) (void)hipHostFree(h->pinned);
            h->pinned = nullptr;
            h->pinned_cap = 0;
            if (hipHostMalloc((void **)&h->pinned, (size_t)padded, hipHostMallocDefault) != hipSuccess) return ing_nomem(h, padded, "pinned staging");
            h->pinned_cap = padded;
        }
        std::memcpy(h->pinned, bytes + off, (size_t)len);
        GH_HIP(hipMemcpyAsync(h->d_text.p, h->pinned, (size_t)len, hipMemcpyHostToDevice, h->stream));
        text = h->d_text.p; lo = 0; cap = h->text_cap;
    }
    const int64_t hi = lo + len, n_words = (hi + 15) / 16 - lo / 16;
    gh_dev<int32_t> d_counts, d_offs;
    if (!d_counts.alloc(4 * (size_t)n_words) || !d_offs.alloc(4 * (size_t)n_words)) return ing_nomem(h, 8 * n_words, "line counts");
    ing_starts_kernel<<<dim3(ing_grid(n_words)), dim3(ING_BLOCK), 0, h->stream>>>(text, lo, hi, cap, n_words, 0, d_counts.p, nullptr, nullptr);
    GH_LAUNCH_CHECK();
    GH_TRY_ST(ing_scan(h, d_counts.p, d_offs.p, n_words));
    int64_t n_lines = 0;
    GH_TRY_ST(ing_scan_total(h, d_counts.p, d_offs.p, n_words, &n_lines));
    if (n_lines < 1 || n_lines > len) { h->err = "line-start count " + std::to_string(n_lines) + " is impossible for " + std::to_string(len) + " bytes"; return GH_ERR_RUNTIME; }
    gh_dev<uint32_t> d_starts;
    gh_dev<int64_t> d_ab;
    gh_dev<int32_t> d_is_row, d_pos;
    if (!d_starts.alloc(4 * (size_t)n_lines) || !d_ab.alloc(16 * (size_t)n_lines) || !d_is_row.alloc(4 * (size_t)n_lines) ||
        !d_pos.alloc(4 * (size_t)n_lines))
        return ing_nomem(h, 28 * n_lines, "parsed lines");
    ing_starts_kernel<<<dim3(ing_grid(n_words)), dim3(ING_BLOCK), 0, h->stream>>>(text, lo, hi, cap, n_words, 1, nullptr, d_offs.p, d_starts.p);
    GH_LAUNCH_CHECK();
    ing_parse_kernel<<<dim3(ing_grid(n_lines)), dim3(ING_BLOCK), 0, h->stream>>>(text + lo, len, off, n_lines, d_starts.p, ingest_comment_byte(format),
                                                                                 format == GH_INGEST_MTX, d_ab.p, d_is_row.p, d_bad.p);
    GH_LAUNCH_CHECK();
    GH_TRY_ST(ing_scan(h, d_is_row.p, d_pos.p, n_lines));
    int64_t n_rows = 0;
    unsigned long long first_bad = ING_NO_ERROR;
    GH_HIP(hipMemcpyAsync(&first_bad, d_bad.p, 8, hipMemcpyDeviceToHost, h->stream));
    GH_TRY_ST(ing_scan_total(h, d_is_row.p, d_pos.p, n_lines, &n_rows));
    *bad = first_bad;
    if (first_bad != ING_NO_ERROR) return GH_OK;
    if (h->R + n_rows >= ING_MAX_ROWS) return ing_invalid(h, "2^30 or more rows");
    GH_TRY_ST(ing_rows_room(h, h->R, h->R + n_rows));
    ing_compact_kernel<<<dim3(ing_grid(n_lines)), dim3(ING_BLOCK), 0, h->stream>>>(n_lines, d_ab.p, d_is_row.p, d_pos.p, h->d_rows.p + 2 * h->R);
    GH_LAUNCH_CHECK();
    GH_HIP(hipStreamSynchronize(h->stream));   // the chunk's buffers go out of scope
    h->R += n_rows;
    return GH_OK;
}

// d_rows (R rows) -> d_vertices and, undirected, d_ids.
gh_status ing_finish_device(gh_ingest *h, bool directed, bool from_rows) {
    const int64_t R = h->R, L = 2 * R;
    h->E = 0;
    h->n_vertices = 0;
    if (R == 0) return GH_OK;
    gh_dev<uint64_t> d_a, d_b;
    gh_dev<int32_t> d_num;
    if (!d_a.alloc(8 * (size_t)L) || !d_b.alloc(8 * (size_t)L) || !d_num.alloc(4)) return ing_nomem(h, 16 * L, "label keys");
    ing_flip_kernel<<<dim3(ing_grid(L)), dim3(ING_BLOCK), 0, h->stream>>>(L, (const uint64_t *)h->d_rows.p, d_a.p);
    GH_LAUNCH_CHECK();
    uint64_t *table = nullptr;
    int64_t n_table = 0;
    GH_TRY_ST(ing_sort_unique(h, d_a.p, d_b.p, L, d_num.p, &table, &n_table));
    if (n_table > 0x7FFFFFFFll) return ing_invalid(h, "more than 2^31 - 1 distinct labels");
    if (directed) {
        if (!h->d_vertices.alloc(8 * (size_t)n_table)) return ing_nomem(h, 8 * n_table, "vertices");
        ing_vertices_kernel<<<dim3(ing_grid(n_table)), dim3(ING_BLOCK), 0, h->stream>>>(n_table, table, nullptr, nullptr, h->d_vertices.p);
        GH_LAUNCH_CHECK();
        GH_HIP(hipStreamSynchronize(h->stream));
        h->E = R;
        h->n_vertices = n_table;
        return GH_OK;
    }
    gh_dev<uint64_t> d_k0, d_k1;
    if (!d_k0.alloc(8 * (size_t)R) || !d_k1.alloc(8 * (size_t)R)) return ing_nomem(h, 16 * R, "edge keys");
    ing_keys_kernel<<<dim3(ing_grid(R)), dim3(ING_BLOCK), 0, h->stream>>>(R, (const uint64_t *)h->d_rows.p, table, n_table, d_k0.p);
    GH_LAUNCH_CHECK();
    uint64_t *keys = nullptr;
    int64_t E = 0;
    GH_TRY_ST(ing_sort_unique(h, d_k0.p, d_k1.p, R, d_num.p, &keys, &E));
    uint64_t last = 0;
    GH_HIP(hipMemcpyAsync(&last, keys + E - 1, 8, hipMemcpyDeviceToHost, h->stream));   // E >= 1 as R >= 1
    GH_HIP(hipStreamSynchronize(h->stream));
    if (last == ING_NO_ERROR) --E;              // the self-loops
    gh_dev<int32_t> d_used, d_rank;
    int64_t n_vertices = n_table;
    if (!from_rows) {
        if (!d_used.alloc(4 * (size_t)n_table) || !d_rank.alloc(4 * (size_t)n_table)) return ing_nomem(h, 8 * n_table, "vertex flags");
        GH_HIP(hipMemsetAsync(d_used.p, 0, 4 * (size_t)n_table, h->stream));
        ing_mark_kernel<<<dim3(ing_grid(E)), dim3(ING_BLOCK), 0, h->stream>>>(E, keys, d_used.p);
        GH_LAUNCH_CHECK();
        GH_TRY_ST(ing_scan(h, d_used.p, d_rank.p, n_table));
        GH_TRY_ST(ing_scan_total(h, d_used.p, d_rank.p, n_table, &n_vertices));
    }
    if (!h->d_vertices.alloc(8 * (size_t)n_vertices) || !h->d_ids.alloc(8 * (size_t)E)) return ing_nomem(h, 8 * (n_vertices + E), "the result");
    ing_vertices_kernel<<<dim3(ing_grid(n_table)), dim3(ING_BLOCK), 0, h->stream>>>(n_table, table, from_rows ? nullptr : d_used.p,
                                                                                    from_rows ? nullptr : d_rank.p, h->d_vertices.p);
    GH_LAUNCH_CHECK();
    ing_ids_kernel<<<dim3(ing_grid(E)), dim3(ING_BLOCK), 0, h->stream>>>(E, keys, from_rows ? nullptr : d_rank.p, h->d_ids.p);
    GH_LAUNCH_CHECK();
    GH_HIP(hipStreamSynchronize(h->stream));
    h->E = E;
    h->n_vertices = n_vertices;
    h->d_rows.reset();                          // an undirected result no longer needs the rows
    h->rows_cap = 0;
    return GH_OK;
}

gh_status ing_parse(gh_ingest *h, const uint8_t *bytes, const uint8_t *d_bytes, int64_t nbytes, int format, int directed, int vertices_from) {
    if (!h) { g_ingest_error = "handle is NULL"; return GH_ERR_INVALID; }
    h->parsed = false;
    if (nbytes < 0 || (nbytes > 0 && !bytes)) return ing_invalid(h, "bytes is NULL or nbytes is negative");
    if (format != GH_INGEST_SNAP && format != GH_INGEST_EDGES && format != GH_INGEST_MTX) return ing_invalid(h, "unknown format " + std::to_string(format));
    if (vertices_from != GH_INGEST_FROM_EDGES && vertices_from != GH_INGEST_FROM_ROWS)
        return ing_invalid(h, "unknown vertices_from " + std::to_string(vertices_from));
    if (d_bytes && h->device < 0) return ing_invalid(h, "a host-path handle takes host bytes only");
    if (d_bytes && ((uintptr_t)d_bytes & 15)) return ing_invalid(h, "d_bytes must be 16-byte aligned");
    const int64_t data_off = ingest_data_offset(bytes, nbytes, format);
    h->directed = directed != 0;
    h->chunks = 0;
    if (h->device < 0) {
        std::vector<int64_t> rows;
        const int64_t bad = ingest_host_rows(bytes, nbytes, data_off, format, &rows);
        if (bad >= 0) return ing_invalid(h, ingest_error_text(bytes, nbytes, bad, format));
        if ((int64_t)rows.size() / 2 >= ING_MAX_ROWS) return ing_invalid(h, "2^30 or more rows");
        GH_TRY_ST(ingest_host_finish(std::move(rows), directed != 0, vertices_from == GH_INGEST_FROM_ROWS, &h->host, &h->err));
        h->R = h->host.R;
        h->E = h->host.E;
        h->n_vertices = (int64_t)h->host.vertices.size();
        h->parsed = true;
        return GH_OK;
    }
    GH_HIP(hipSetDevice(h->device));
    h->R = 0;
    h->d_ids.reset();
    h->d_vertices.reset();
    gh_dev<unsigned long long> d_bad;
    if (!d_bad.alloc(8)) return ing_nomem(h, 8, "the error word");
    GH_HIP(hipMemsetAsync(d_bad.p, 0xFF, 8, h->stream));
    const int64_t chunk = ing_chunk_bytes(h);
    for (int64_t off = data_off; off < nbytes;) {
        const int64_t end = ingest_chunk_end(bytes, nbytes, off, chunk);
        if (end - off > 0x7FFFFFFFll) return ing_invalid(h, "a line of 2^31 bytes or more");
        uint64_t bad = ING_NO_ERROR;
        ++h->chunks;
        GH_TRY_ST(ing_chunk(h, bytes, d_bytes, nbytes, off, end, format, d_bad, &bad));
        if (bad != ING_NO_ERROR) return ing_invalid(h, ingest_error_text(bytes, nbytes, (int64_t)bad, format));
        off = end;
    }
    GH_TRY_ST(ing_finish_device(h, directed != 0, vertices_from == GH_INGEST_FROM_ROWS));
    h->parsed = true;
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_ingest_create(gh_ingest_handle *out, int device_id) {
    if (!out) { g_ingest_error = "out is NULL"; return GH_ERR_INVALID; }
    *out = nullptr;
    gh_ingest *h = new gh_ingest();
    h->budget = ING_DEFAULT_BUDGET;
    if (device_id >= 0) {
        const gh_status st = gh_host_open(h, device_id, &g_ingest_error);
        if (st != GH_OK) { gh_ingest_destroy(h); return st; }
    }
    *out = h;
    return GH_OK;
}

extern "C" void gh_ingest_destroy(gh_ingest_handle h) {
    if (!h) return;
    gh_host_close(h);
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
}

extern "C" const char *gh_ingest_last_error(gh_ingest_handle h) { return h ? h->err.c_str() : g_ingest_error.c_str(); }

extern "C" gh_status gh_ingest_set_memory_budget(gh_ingest_handle h, int64_t bytes) {
    if (h && bytes > 0 && bytes < GH_INGEST_MIN_BUDGET) return ing_invalid(h, "budget must be 0 (the default) or at least " + std::to_string(GH_INGEST_MIN_BUDGET));
    return gh_host_set_budget(h, bytes, ING_DEFAULT_BUDGET, &g_ingest_error);
}

extern "C" gh_status gh_ingest_parse(gh_ingest_handle h, const uint8_t *bytes, int64_t nbytes, int32_t format, int32_t directed,
                                     int32_t vertices_from) {
    return ing_parse(h, bytes, nullptr, nbytes, format, directed, vertices_from);
}

extern "C" gh_status gh_ingest_parse_uploaded(gh_ingest_handle h, const uint8_t *bytes, const uint8_t *d_bytes, int64_t nbytes, int32_t format,
                                              int32_t directed, int32_t vertices_from) {
    if (h && nbytes > 0 && !d_bytes) return ing_invalid(h, "d_bytes is NULL");
    return ing_parse(h, bytes, nbytes > 0 ? d_bytes : nullptr, nbytes, format, directed, vertices_from);
}

extern "C" gh_status gh_ingest_counts(gh_ingest_handle h, int64_t *rows, int64_t *edges, int64_t *vertices) {
    if (!h) { g_ingest_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (!h->parsed) return ing_invalid(h, "nothing was parsed");
    if (rows) *rows = h->R;
    if (edges) *edges = h->E;
    if (vertices) *vertices = h->n_vertices;
    return GH_OK;
}

extern "C" gh_status gh_ingest_chunking(gh_ingest_handle h, int64_t *chunk_bytes, int64_t *chunks) {
    if (!h) { g_ingest_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (chunk_bytes) *chunk_bytes = ing_chunk_bytes(h);
    if (chunks) *chunks = h->chunks;
    return GH_OK;
}

extern "C" gh_status gh_ingest_copy_vertices(gh_ingest_handle h, int64_t *vertices) {
    if (!h) { g_ingest_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (!h->parsed) return ing_invalid(h, "nothing was parsed");
    if (h->n_vertices == 0) return GH_OK;
    if (!vertices) return ing_invalid(h, "vertices is NULL");
    if (h->device < 0) { std::copy(h->host.vertices.begin(), h->host.vertices.end(), vertices); return GH_OK; }
    GH_HIP(hipSetDevice(h->device));
    GH_HIP(hipMemcpyAsync(vertices, h->d_vertices.p, 8 * (size_t)h->n_vertices, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_ingest_copy_edges(gh_ingest_handle h, int32_t relabel, int64_t *edges) {
    if (!h) { g_ingest_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (!h->parsed) return ing_invalid(h, "nothing was parsed");
    if (h->E == 0) return GH_OK;
    if (!edges) return ing_invalid(h, "edges is NULL");
    if (h->device < 0) { ingest_host_edges(h->host, relabel != 0, edges); return GH_OK; }
    GH_HIP(hipSetDevice(h->device));
    const int64_t count = 2 * h->E;
    if (h->directed && !relabel) {
        GH_HIP(hipMemcpyAsync(edges, h->d_rows.p, 8 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        return GH_OK;
    }
    gh_dev<int64_t> d_out;
    if (!d_out.alloc(8 * (size_t)count)) return ing_nomem(h, 8 * count, "edges");
    ing_edges_out_kernel<<<dim3(ing_grid(count)), dim3(ING_BLOCK), 0, h->stream>>>(count, h->directed ? nullptr : h->d_ids.p, h->d_rows.p,
                                                                                  h->d_vertices.p, h->n_vertices, relabel != 0, d_out.p);
    GH_LAUNCH_CHECK();
    GH_HIP(hipMemcpyAsync(edges, d_out.p, 8 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}
