// The edge-list parsing rule (include/graphem_hip.h "edge-list ingestion") in one place: the line parser that the
// kernels and the host path both compile, and the whole host path in plain C++.  Nothing here needs the HIP headers, so a
// host compiler alone builds it (tools/ingest_host_check.cpp runs it under the sanitizers).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"

#ifdef __HIPCC__
#define GH_INGEST_HD __host__ __device__ __forceinline__
#else
#define GH_INGEST_HD inline
#endif

enum { INGEST_SKIP = 0, INGEST_ROW = 1, INGEST_BAD_INT = 2, INGEST_BAD_RANGE = 3 };

GH_INGEST_HD bool ingest_blank(uint8_t c) { return c == 0x09 || c == 0x0B || c == 0x0C || (c >= 0x1C && c <= 0x20); }

// The field [p, p + n) as [+-]?[0-9]+ in int64, less dec (0 or 1).  A bad byte wins over an overflow.
GH_INGEST_HD int ingest_int(const uint8_t *p, int64_t n, int dec, int64_t *out) {
    int64_t i = 0;
    bool neg = false;
    if (n > 0 && (p[0] == '+' || p[0] == '-')) { neg = p[0] == '-'; i = 1; }
    if (i >= n) return INGEST_BAD_INT;
    const uint64_t limit = neg ? (1ull << 63) : (1ull << 63) - 1;
    uint64_t mag = 0;
    bool over = false;
    for (; i < n; ++i) {
        const unsigned d = (unsigned)p[i] - (unsigned)'0';
        if (d > 9) return INGEST_BAD_INT;
        if (mag > (limit - d) / 10) over = true;    // mag * 10 + d would pass the limit
        else mag = mag * 10 + d;
    }
    if (over) return INGEST_BAD_RANGE;
    int64_t v = (int64_t)(neg ? 0 - mag : mag);
    if (dec) {
        if (v == INT64_MIN) return INGEST_BAD_RANGE;
        v -= 1;
    }
    *out = v;
    return INGEST_ROW;
}

// One line [p, p + n), its terminator included or not.  comment: the byte that makes the line a comment when it comes
// first, or -1.  A bad line leaves the offending field in [*bad_at, *bad_at + *bad_len).  Reads nothing outside the line.
GH_INGEST_HD int ingest_parse_line(const uint8_t *p, int64_t n, int comment, int dec, int64_t *a, int64_t *b,
                                   int64_t *bad_at, int64_t *bad_len) {
    while (n > 0 && (p[n - 1] == '\n' || p[n - 1] == '\r')) --n;
    if (comment >= 0 && n > 0 && p[0] == (uint8_t)comment) return INGEST_SKIP;
    int64_t i = 0;
    while (i < n && ingest_blank(p[i])) ++i;
    const int64_t s0 = i;
    while (i < n && !ingest_blank(p[i])) ++i;
    const int64_t e0 = i;
    while (i < n && ingest_blank(p[i])) ++i;
    const int64_t s1 = i;
    while (i < n && !ingest_blank(p[i])) ++i;
    const int64_t e1 = i;
    if (e1 == s1) return INGEST_SKIP;               // fewer than two fields
    int k = ingest_int(p + s0, e0 - s0, dec, a);
    if (k != INGEST_ROW) { *bad_at = s0; *bad_len = e0 - s0; return k; }
    k = ingest_int(p + s1, e1 - s1, dec, b);
    if (k != INGEST_ROW) { *bad_at = s1; *bad_len = e1 - s1; return k; }
    return INGEST_ROW;
}

GH_INGEST_HD int ingest_comment_byte(int format) { return format == GH_INGEST_MTX ? -1 : '#'; }

// ---- host side ------------------------------------------------------------------------------------------------------

// The offset just after the terminator of the line that holds `pos`, or n.
inline int64_t ingest_line_end(const uint8_t *t, int64_t n, int64_t pos) {
    while (pos < n && t[pos] != '\n' && t[pos] != '\r') ++pos;
    if (pos >= n) return n;
    if (t[pos] == '\r' && pos + 1 < n && t[pos + 1] == '\n') return pos + 2;
    return pos + 1;
}

// Where the data of a file begins: 0, or for mtx after the leading '%' lines and the one line that follows them.
inline int64_t ingest_data_offset(const uint8_t *t, int64_t n, int format) {
    if (format != GH_INGEST_MTX) return 0;
    int64_t pos = 0;
    while (pos < n) {
        const bool comment = t[pos] == '%';
        pos = ingest_line_end(t, n, pos);
        if (!comment) break;
    }
    return pos;
}

// Where the chunk that begins at `off` ends: the last offset in (off, off + chunk] that follows a whole terminator; when
// the line at `off` is longer than that, the end of that line.
inline int64_t ingest_chunk_end(const uint8_t *t, int64_t n, int64_t off, int64_t chunk) {
    if (n - off <= chunk) return n;
    int64_t e = off + chunk;                        // e < n
    while (e > off && !(t[e - 1] == '\n' || (t[e - 1] == '\r' && t[e] != '\n'))) --e;
    return e > off ? e : ingest_line_end(t, n, off + chunk);
}

// The message for the bad line that begins at line_off.
inline std::string ingest_error_text(const uint8_t *t, int64_t n, int64_t line_off, int format) {
    int64_t line = 1;
    for (int64_t pos = 0; pos < line_off; ++line) pos = ingest_line_end(t, n, pos);
    const int64_t end = ingest_line_end(t, n, line_off);
    int64_t a, b, at = 0, len = 0;
    const int k = ingest_parse_line(t + line_off, end - line_off, ingest_comment_byte(format), format == GH_INGEST_MTX, &a, &b, &at, &len);
    const std::string field((const char *)t + line_off + at, (size_t)std::min<int64_t>(len, 80));
    return "line " + std::to_string(line) + (k == INGEST_BAD_RANGE ? ": integer outside int64 '" : ": invalid integer '") + field + "'";
}

// All data rows of [data_off, n) in file order as (a, b) pairs in *rows.  Returns the offset of the first bad line, or -1.
inline int64_t ingest_host_rows(const uint8_t *t, int64_t n, int64_t data_off, int format, std::vector<int64_t> *rows) {
    const int comment = ingest_comment_byte(format), dec = format == GH_INGEST_MTX;
    rows->clear();
    for (int64_t pos = data_off; pos < n;) {
        const int64_t end = ingest_line_end(t, n, pos);
        int64_t a = 0, b = 0, at, len;
        const int k = ingest_parse_line(t + pos, end - pos, comment, dec, &a, &b, &at, &len);
        if (k >= INGEST_BAD_INT) return pos;
        if (k == INGEST_ROW) { rows->push_back(a); rows->push_back(b); }
        pos = end;
    }
    return -1;
}

// What a parse leaves behind on the host path: the vertices, and the edges either as the rows' labels (directed) or as
// pairs of ranks in `vertices` (undirected).
struct ingest_result {
    std::vector<int64_t> vertices, rows;
    std::vector<int32_t> ids;
    int64_t R = 0, E = 0;
};

inline gh_status ingest_host_finish(std::vector<int64_t> &&rows, bool directed, bool from_rows, ingest_result *res, std::string *err) {
    res->R = (int64_t)rows.size() / 2;
    res->ids.clear();
    std::vector<int64_t> table(rows);
    std::sort(table.begin(), table.end());
    table.erase(std::unique(table.begin(), table.end()), table.end());
    if (table.size() > 0x7FFFFFFFull) { *err = "more than 2^31 - 1 distinct labels"; return GH_ERR_INVALID; }
    if (directed) {
        res->vertices = std::move(table);
        res->rows = std::move(rows);
        res->E = res->R;
        return GH_OK;
    }
    std::vector<uint64_t> keys;
    keys.reserve((size_t)res->R);
    for (int64_t r = 0; r < res->R; ++r) {
        const uint64_t u = (uint64_t)(std::lower_bound(table.begin(), table.end(), rows[2 * r]) - table.begin());
        const uint64_t v = (uint64_t)(std::lower_bound(table.begin(), table.end(), rows[2 * r + 1]) - table.begin());
        if (u != v) keys.push_back((std::min(u, v) << 32) | std::max(u, v));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    res->rows.clear();
    res->E = (int64_t)keys.size();
    std::vector<int32_t> rank(table.size());
    if (from_rows) {
        for (size_t i = 0; i < table.size(); ++i) rank[i] = (int32_t)i;
        res->vertices = std::move(table);
    } else {
        std::vector<uint8_t> used(table.size(), 0);
        for (uint64_t k : keys) used[k >> 32] = used[k & 0xFFFFFFFFull] = 1;
        res->vertices.clear();
        for (size_t i = 0; i < table.size(); ++i) {
            rank[i] = (int32_t)res->vertices.size();
            if (used[i]) res->vertices.push_back(table[i]);
        }
    }
    res->ids.resize(2 * keys.size());
    for (size_t e = 0; e < keys.size(); ++e) {
        res->ids[2 * e] = rank[keys[e] >> 32];
        res->ids[2 * e + 1] = rank[keys[e] & 0xFFFFFFFFull];
    }
    return GH_OK;
}

// edges (E, 2) int64 of a host result: labels, or ranks in vertices when relabel.
inline void ingest_host_edges(const ingest_result &res, bool relabel, int64_t *out) {
    if (!res.ids.empty() || res.rows.empty()) {
        for (size_t i = 0; i < res.ids.size(); ++i) out[i] = relabel ? (int64_t)res.ids[i] : res.vertices[res.ids[i]];
        return;
    }
    for (size_t i = 0; i < res.rows.size(); ++i)
        out[i] = relabel ? (int64_t)(std::lower_bound(res.vertices.begin(), res.vertices.end(), res.rows[i]) - res.vertices.begin()) : res.rows[i];
}
